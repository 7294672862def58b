"""A float64 reference of the k = 4x4(x kt), stride (1,2,2), pad (0,1,1) convolution that scales to the benchmark's batch sizes, and a
comparator that says WHICH tile of a result is wrong.

The reference works tap by tap in the device layout (x [N][T][H][W][Ci], w [Co][kt][4][4][Ci], y [N][To][Ho][Wo][Co]) on torch
tensors of any device: per tap one strided slice of the padded input and one dense matmul -- no im2col array, memory a few times
the tensors themselves.  Nothing of the package is involved.  (oracle.functions.conv3d_* builds the im2col array: several GB in
float64 at 64 clips; tests/test_ref64_cpu.py pins this module to it and to torch.nn.functional.conv3d at small sizes.)

The comparator works on device tensors: global rel-L2, and a localised error over blocks of 256 rows x 64 columns of the result seen
as the GEMM's [M][C] matrix,
    ||got - ref||_block / (||ref||_global * sqrt(block_size / size)),
i.e. the block's error against the reference norm an average block of its size holds.  A correct kernel's rounding error is spread
evenly, so its blocks scatter around the global value; a dropped K-step, a tile written to the wrong rows or a missing split-K
addend puts >= 1e-2 into one block while the global figure over 200 000 rows stays below 1e-5."""
import torch

F64 = torch.float64
BLOCK_ROWS, BLOCK_COLS = 256, 64
BLOCK_FACTOR = 4.0          # worst block must stay below BLOCK_FACTOR x the tolerance of the global rel-L2 (a condition, not a measurement)


def _pad_hw(x):
    N, T, H, W, C = x.shape
    xp = x.new_zeros((N, T, H + 2, W + 2, C))
    xp[:, :, 1:H + 1, 1:W + 1] = x
    return xp


def _taps(kt):
    return [(a, kh, kw) for a in range(kt) for kh in range(4) for kw in range(4)]


def fprop(x, w, bias=None, dtype=F64):
    """y[N,To,Ho,Wo,Co] = conv(x[N,T,H,W,Ci], w[Co,kt,4,4,Ci]) + bias; H and W independent (even)."""
    x, w = x.to(dtype), w.to(dtype)
    N, T, H, W, Ci = x.shape
    Co, kt = w.shape[0], w.shape[1]
    To, Ho, Wo = T - kt + 1, H // 2, W // 2
    xp = _pad_hw(x)
    y = x.new_zeros((N * To * Ho * Wo, Co))
    for a, kh, kw in _taps(kt):
        y += xp[:, a:a + To, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :].reshape(-1, Ci) @ w[:, a, kh, kw, :].T
    if bias is not None:
        y += bias.to(dtype)
    return y.view(N, To, Ho, Wo, Co)


def dgrad(gy, w, T, H, W, dtype=F64):
    """gx[N,T,H,W,Ci]: the transposed scatter of the same taps into a padded gx, borders cut off."""
    gy, w = gy.to(dtype), w.to(dtype)
    N, To, Ho, Wo, Co = gy.shape
    kt, Ci = w.shape[1], w.shape[4]
    assert To == T - kt + 1 and Ho == H // 2 and Wo == W // 2
    gxp = gy.new_zeros((N, T, H + 2, W + 2, Ci))
    g2 = gy.reshape(-1, Co)
    for a, kh, kw in _taps(kt):
        gxp[:, a:a + To, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :] += (g2 @ w[:, a, kh, kw, :]).view(N, To, Ho, Wo, Ci)
    return gxp[:, :, 1:H + 1, 1:W + 1].contiguous()


def wgrad(x, gy, kt, dtype=F64):
    """dw[Co,kt,4,4,Ci] = sum over pixels of gy (x) the tap's input."""
    x, gy = x.to(dtype), gy.to(dtype)
    N, T, H, W, Ci = x.shape
    _, To, Ho, Wo, Co = gy.shape
    assert To == T - kt + 1 and Ho == H // 2 and Wo == W // 2
    xp = _pad_hw(x)
    g2t = gy.reshape(-1, Co).T
    dw = x.new_zeros((Co, kt, 4, 4, Ci))
    for a, kh, kw in _taps(kt):
        dw[:, a, kh, kw, :] = g2t @ xp[:, a:a + To, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :].reshape(-1, Ci)
    return dw


class Report:
    """what compare() found: .rel (global rel-L2), .block (worst localised error), .rows / .cols (that block's half-open ranges)"""

    def __init__(self, rel, block, rows, cols, shape):
        self.rel, self.block, self.rows, self.cols, self.shape = rel, block, rows, cols, shape

    def ok(self, tol):
        return self.rel < tol and self.block < BLOCK_FACTOR * tol

    def __str__(self):
        return "rel-L2 %.2e, worst block %.2e at rows %d..%d cols %d..%d of [%d][%d]" % (
            (self.rel, self.block) + self.rows + self.cols + self.shape)


def compare(got, ref, cols=None, row_chunk=None):
    """got, ref: tensors of one shape on one device, seen as [M][C] with C = the last dimension (cols=: another row length, for a
    filter gradient [Co][kt*16*Ci]).  Works in chunks of rows: no float64 copy of the whole of `got`."""
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    C = got.shape[-1] if cols is None else cols
    g2, r2 = got.reshape(-1, C), ref.reshape(-1, C)
    M = g2.shape[0]
    nbr, nbc = -(-M // BLOCK_ROWS), -(-C // BLOCK_COLS)
    err2 = torch.zeros((nbr, nbc), dtype=F64, device=ref.device)
    ref2 = torch.zeros((), dtype=F64, device=ref.device)
    if row_chunk is None:
        row_chunk = (1 << 25) // (nbc * BLOCK_COLS)                     # float64 temporaries of 256 MB
    row_chunk = max(BLOCK_ROWS, row_chunk // BLOCK_ROWS * BLOCK_ROWS)
    for r0 in range(0, M, row_chunk):
        r1 = min(M, r0 + row_chunk)
        r = r2[r0:r1].to(F64)
        d = (g2[r0:r1].to(F64) - r) ** 2
        d = torch.nan_to_num(d, nan=float('inf'))                      # a NaN in `got` must fail the comparison, not vanish from it
        ref2 += (r * r).sum()
        pr, pc = -(r1 - r0) % BLOCK_ROWS, -C % BLOCK_COLS
        if pr or pc:
            d = torch.nn.functional.pad(d, (0, pc, 0, pr))
        err2[r0 // BLOCK_ROWS:r0 // BLOCK_ROWS + d.shape[0] // BLOCK_ROWS] = d.view(-1, BLOCK_ROWS, nbc, BLOCK_COLS).sum(dim=(1, 3))
    ref_norm = max(float(ref2.sqrt()), 1e-300)
    # sizes of the blocks (the last row / column block may be partial)
    rs = torch.full((nbr,), BLOCK_ROWS, dtype=F64, device=ref.device)
    cs = torch.full((nbc,), BLOCK_COLS, dtype=F64, device=ref.device)
    rs[-1], cs[-1] = M - (nbr - 1) * BLOCK_ROWS, C - (nbc - 1) * BLOCK_COLS
    size = rs[:, None] * cs[None, :]
    local = err2.sqrt() / (ref_norm * (size / float(M * C)).sqrt())
    i = int(local.argmax())
    br, bc = i // nbc, i % nbc
    return Report(float(err2.sum().sqrt()) / ref_norm, float(local[br, bc]),
                  (br * BLOCK_ROWS, min(M, (br + 1) * BLOCK_ROWS)), (bc * BLOCK_COLS, min(C, (bc + 1) * BLOCK_COLS)), (M, C))
