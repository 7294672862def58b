"""MI355X-native MoCoGAN training hot path.

``csrc/``      hand-written HIP kernels for gfx950 + the C ABI declared in ``include/mocogan_hip.h``
``hiplib.py``  ctypes binding of ``lib/libmocogan_hip.so`` (raw device pointers, current HIP stream)
``tiles.py``   which GEMM tile a conv launch takes: candidate rules, the tile table, the shipped lists, the tuning loop (no torch)
``layout.py``  reference (Chainer) layout <-> device layout of activations and parameters
``nets.py``    ImageGenerator / ImageDiscriminator / VideoDiscriminator on those kernels
``step.py``    one training iteration (losses, hand-scheduled backward, Adam) + data-parallel exchange
``metrics.py`` sliced Wasserstein distance between two sets of uint8 clips (evaluate_swd.py); nearest-neighbour precision / recall,
             density / coverage and a data-copying score on the int8 matrix pipe (evaluate_knn.py); content distance, lag profile, motion k-NN
             figures and the content x motion grid (evaluate_motion.py)
The reference-facing API (``model.net``, ``model.updater``, ``train.py``) at the repo root is a
thin layer over these modules.
"""
from .build import build, lib_path  # noqa: F401
