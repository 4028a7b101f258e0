"""Reference pieces shared by test_transpose_cpu.py and test_transpose_gpu.py:
the error bounds of the issue and a torch emulation of transpose.hip's
chunked column sum (csrc/kernels/transpose.hip)."""
import torch

TILE = 128          # rows per tile in transpose.hip
SHAPES = [(8, 8), (64, 64), (72, 136), (200, 264), (1032, 4096)]


def colsum_bound(x):
    """(ref, bound) for column sums of bf16 x [R, C]:
    |out - ref| <= 2^-8 |ref| + R 2^-24 sum_r |x|: bf16 rounding of the
    result plus the worst fp32 summation error in any order."""
    xd = x.double()
    ref = xd.sum(0)
    return ref, 2.0 ** -8 * ref.abs() + x.shape[0] * 2.0 ** -24 * xd.abs().sum(0)


def wgrad_bound(x, dy):
    """(ref, bound) for dw = x^T dy of bf16 x [T, in], dy [T, out]:
    |out - ref| <= 2^-8 |ref| + T 2^-24 sum_t |x||dy|.  bf16 products are
    exact in fp32, so this holds for any accumulation order."""
    xd, dd = x.double(), dy.double()
    ref = xd.t() @ dd
    return ref, 2.0 ** -8 * ref.abs() + x.shape[0] * 2.0 ** -24 * (xd.abs().t() @ dd.abs())


def plan(r, c):
    """transpose_plan of transpose.hip: (tiles_per_chunk, chunks)."""
    xblocks = -(-c // TILE)
    nrt = -(-r // TILE)
    want = min(nrt, max(1, 2048 // xblocks))
    tpc = -(-nrt // want)
    return tpc, -(-nrt // tpc)


def chunked_colsum(x, tiles_per_chunk=None, drop_last_partial_tile=False,
                   drop_chunk=None, over_output_columns=False):
    """fp32 column sums of x [R, C] the way the kernel forms them: per chunk
    of row tiles, 16 row groups of 8 rows per tile added in row order, the
    groups added in order, then the chunks in order.  The keyword arguments
    plant the mistakes test_transpose_cpu.py must catch."""
    r, c = x.shape
    tpc, chunks = plan(r, c)
    if tiles_per_chunk is not None:
        tpc = tiles_per_chunk
        chunks = -(-(-(-r // TILE)) // tpc)
    if over_output_columns:
        # sums over the columns of the output [C, R], i.e. over input rows'
        # wrong axis: one value per input row
        return x.float().sum(1)
    rows = r
    if drop_last_partial_tile and r % TILE:
        rows = r - r % TILE
    xf = x.float()
    parts = []
    for ch in range(chunks):
        r0, r1 = ch * tpc * TILE, min(rows, (ch + 1) * tpc * TILE)
        acc = torch.zeros(16, c, dtype=torch.float32)
        for row in range(r0, max(r0, r1)):
            acc[(row % TILE) // 8] += xf[row]
        part = torch.zeros(c, dtype=torch.float32)
        for g in range(16):
            part += acc[g]
        parts.append(part)
    out = torch.zeros(c, dtype=torch.float32)
    for ch, part in enumerate(parts):
        if ch != drop_chunk:
            out += part
    return out
