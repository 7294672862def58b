"""Records tests/golden/step_launch_trace.json: what TrainStep.run enqueues, per configuration of tests/test_gpu_step_trace.py.

    python tests/golden/make_step_launch_trace.py --commit <revision of the package that is recorded> [--out FILE] [--reversed]

Needs an MI355X.  The file in the repository was recorded from commit e35d39e, the parent of the commit that split run() into
phases: a checkout of that commit, built, with tests/launch_trace.py, tests/test_gpu_step_trace.py and this script copied into it
(they use nothing the older package lacks), run there.  It is the yardstick for later changes of run() and is NOT re-recorded from
a tree to make that tree's test pass: a trace that differs is a finding about the change.  A change that means to alter the
schedule records a new file from its own parent first, shows the differing entries, and then records its own.
--reversed records the configurations in the opposite order (the traces must not depend on what ran before in the process)."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import launch_trace                        # noqa: E402
import test_gpu_step_trace as case         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', required=True)
    ap.add_argument('--out', default=case.GOLDEN)
    ap.add_argument('--reversed', action='store_true')
    args = ap.parse_args()
    names = sorted(case.CONFIGS, reverse=args.reversed)
    traces = {name: case.record(name) for name in names}
    launch_trace.save(args.out, {name: traces[name] for name in sorted(traces)}, recorded_from=args.commit,
                      recorder='tests/launch_trace.py', iterations=2)
    for name in sorted(traces):
        print(name, len(traces[name]), 'entries')


if __name__ == '__main__':
    main()
