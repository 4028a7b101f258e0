"""Reference for test_moe_permute_cpu.py and test_moe_permute_gpu.py: the
route as a Python loop, dispatch / combine and their gradients in fp64 torch,
the error bounds, and the checks both files run on their device through the
public functions of paddle_amd.ops.functional."""
import torch

from paddle_amd.ops import functional as hot

# (T, K, E, cap, h): drops | empty tails, one 16-byte piece | T past a chunk,
# ragged row | K = 4 | single token
SHAPES = [(150, 2, 4, 5, 64), (150, 2, 4, 200, 8), (65, 1, 64, 4, 520),
          (130, 4, 8, 40, 128), (1, 2, 4, 4, 64)]
# (shape, dtype, token 0 with every choice dropped)
CASES = [(s, torch.bfloat16, False) for s in SHAPES] + [
    (SHAPES[0], torch.bfloat16, True), (SHAPES[3], torch.float32, False)]
U = 2.0 ** -24


def rnd(shape, dtype, device, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(device)


def make_topi(T, K, E, bad_token=False, seed=0):
    """Distinct choices per token from [0, E - 1): the last expert is empty.
    bad_token: token 0, which no capacity could drop, gets ids outside [0, E)."""
    g = torch.Generator().manual_seed(seed)
    topi = torch.rand(T, E - 1, generator=g).argsort(1)[:, :K].to(torch.int32)
    if bad_token:
        topi[0] = torch.tensor(([-1, E] * K)[:K])
    return topi.contiguous()


def route_ref(topi, E, cap, restart_per_kk=False):
    T, K = topi.shape
    slot_of = [[-1] * K for _ in range(T)]
    src_of, counts, nxt = [-1] * (E * cap), [0] * E, [0] * E
    for kk in range(K):
        if restart_per_kk:              # planted: the per-(expert, kk) order
            nxt = [0] * E
        for t, row in enumerate(topi.tolist()):
            e = row[kk]
            if 0 <= e < E:
                pos, nxt[e], counts[e] = nxt[e], nxt[e] + 1, counts[e] + 1
                if pos < cap:
                    slot_of[t][kk] = e * cap + pos
                    src_of[e * cap + pos] = t * K + kk
    return [torch.tensor(v, dtype=torch.int32).reshape(shape)
            for v, shape in ((slot_of, (T, K)), (src_of, (-1,)), (counts, (-1,)))]


def dispatch_ref(x, src_of, K, by_mod=False):
    t = src_of % x.shape[0] if by_mod else src_of // K     # planted: src % T
    rows = x[t.clamp(min=0).long()]
    return torch.where((src_of >= 0)[:, None], rows, torch.zeros_like(rows))


def combine_ref(y, w, slot_of, drop_last=False):
    """fp64 (ref, A = sum_kk |w y|)."""
    valid = slot_of >= 0
    if drop_last:                       # planted: the last kk is left out
        valid = valid & (torch.arange(valid.shape[1]) < valid.shape[1] - 1)
    wk = torch.where(valid, w.double(), torch.zeros_like(w, dtype=torch.float64))
    prod = wk[:, :, None] * y.double()[slot_of.clamp(min=0).long()]
    return prod.sum(1), prod.abs().sum(1)


def dy_ref(w, dout, src_of, K):
    g = torch.where(src_of >= 0, w.double().reshape(-1)[src_of.clamp(min=0).long()],
                    torch.zeros_like(src_of, dtype=torch.float64))
    ref = g[:, None] * dout.double()[(src_of // K).clamp(min=0).long()]
    return ref, ref.abs()


def dw_ref(y, dout, slot_of):
    """fp64 (ref, bound): h 2^-24 sum_h |y dout| holds for any order."""
    prod = y.double()[slot_of.clamp(min=0).long()] * dout.double()[:, None, :]
    prod = torch.where((slot_of >= 0)[:, :, None], prod, torch.zeros_like(prod))
    return prod.sum(-1), y.shape[1] * U * prod.abs().sum(-1)


def row_bound(ref, A, K, dtype):
    """One rounding of the result (bf16 rows) + fp32 products and sums."""
    return (2.0 ** -7 * ref.abs() if dtype == torch.bfloat16 else 0) + (K + 1) * U * A


def worst(got, ref, bound):
    """max err / bound (0 / 0 counts as 0, inf outside); <= 1 is inside."""
    err, bound = (got.detach().cpu().double() - ref.cpu()).abs(), bound.cpu()
    ratio = torch.where(err <= bound, err / bound.clamp(min=1e-300),
                        torch.full_like(err, float("inf")))
    return float(ratio.max())


def report(what, figs):
    print(f"moe_permute {what} worst err/bound " + " ".join(f"{k} {v:.3f}" for k, v in figs.items()))
    assert all(v <= 1.0 for v in figs.values()), figs


def stub(xe, inverse=False):
    """Fixed linear 'experts', exact in every dtype: a column rotation and
    signed powers of two.  inverse: its transpose (the backward)."""
    i = torch.arange(xe.shape[1], device=xe.device)
    scale = (2.0 ** (i % 3 - 1) * (1 - 2 * (i % 2))).to(xe.dtype)
    return (xe * scale).roll(3, 1) if not inverse else xe.roll(-3, 1) * scale


def check_case(device, shape, dtype, bad_token):
    """hot.moe_route, then moe_combine(stub(moe_dispatch(x)), w) and its
    backward on `device`: every kernel against the fp64 reference of its own
    inputs; for fp32 rows also the whole chain against fp64 torch autograd of
    the reference (each fp32 value is one product or a sum of K products, so
    the same bounds hold end to end)."""
    T, K, E, cap, h = shape
    topi = make_topi(T, K, E, bad_token)
    slot_r, src_r, cnt_r = route_ref(topi, E, cap)
    slot_of, src_of, counts = hot.moe_route(topi.to(device), E, cap)
    for got, ref in ((slot_of, slot_r), (src_of, src_r), (counts, cnt_r)):
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), ref)
    kept = slot_of[slot_of >= 0]
    assert kept.unique().numel() == kept.numel() == int((src_of >= 0).sum())
    assert int(counts[E - 1]) == 0 and (not bad_token or bool((slot_of[0] < 0).all()))

    x0, dout = rnd((T, h), dtype, "cpu", 1), rnd((T, h), dtype, "cpu", 2)
    w0 = torch.rand(T, K, generator=torch.Generator().manual_seed(3))
    x, w = x0.clone().to(device).requires_grad_(), w0.clone().to(device).requires_grad_()
    xe = hot.moe_dispatch(x, src_of, slot_of)
    y = stub(xe)
    out = hot.moe_combine(y, w, slot_of, src_of)
    xe.retain_grad(), y.retain_grad()
    out.backward(dout.to(device))
    assert torch.equal(xe.detach().cpu(), dispatch_ref(x0, src_r, K))
    assert bool((out[(slot_of < 0).all(1)] == 0).all())
    assert w.grad.dtype == torch.float32 and bool((w.grad[slot_of < 0] == 0).all())
    yc = y.detach().cpu()
    ref, A = combine_ref(yc, w0, slot_r)
    figs = {"out": worst(out, ref, row_bound(ref, A, K, dtype))}
    ref, A = dy_ref(w0, dout, src_r, K)
    figs["dy"] = worst(y.grad, ref, row_bound(ref, A, K, dtype))
    figs["dw"] = worst(w.grad, *dw_ref(yc, dout, slot_r))
    ref, A = combine_ref(xe.grad.cpu(), torch.ones(T, K), slot_r)
    figs["dx"] = worst(x.grad, ref, row_bound(ref, A, K, dtype))
    if dtype == torch.float32:
        xd, wd = x0.double().requires_grad_(), w0.double().requires_grad_()
        yd = stub(dispatch_ref(xd, src_r, K))
        ref, A = combine_ref(yd, wd, slot_r)
        (ref * dout.double()).sum().backward()
        # dx[t] = sum of w[t, kk] stub^T(dout[t]) over kept kk
        a_dx = stub(dout.double(), True).abs() * (w0.double() * (slot_r >= 0)).sum(1, keepdim=True)
        figs["chain out"] = worst(out, ref.detach(), (K + 1) * U * A.detach())
        figs["chain dx"] = worst(x.grad, xd.grad, (K + 1) * U * a_dx)
        figs["chain dw"] = worst(w.grad, wd.grad, dw_ref(yd.detach(), dout, slot_r)[1])
    report(f"{device} {shape} {dtype} bad_token={bad_token}", figs)


def check_layer(device):
    """MoELayer(dispatch="fused"), fp32, tiny config with the capacity cut so
    that entries drop, against the references around the same gate and
    experts.  `back` is the same bits on both sides, so out meets the combine
    bound; the backward graphs differ by fp32 summation order alone (h 2^-24 =
    2^-18 for dw), x.grad is held to 2^-16 of its largest entry: 4x for the
    softmax Jacobian and gate matmul that dw passes through."""
    import paddle_amd as paddle
    from paddle_amd.models.moe import MoELayer
    paddle.seed(0)
    E, K, h = 4, 2, 64
    layer = MoELayer(hidden_size=h, inter_size=128, num_experts=E, k=K,
                     capacity_factor=0.5, dispatch="fused").to(device=device)
    x = rnd((2, 16, h), torch.float32, device, 9).requires_grad_()
    gout = rnd((2, 16, h), torch.float32, device, 10)
    out = layer(x)
    (out * gout).sum().backward()

    x2 = x.detach().clone().requires_grad_()
    tokens = x2.reshape(-1, h)
    topv, topi, _ = layer.gate(tokens)
    cap = int(0.5 * 32 * K / E) + 1
    slot_r, src_r, counts = route_ref(topi.cpu().to(torch.int32), E, cap)
    assert int(counts.max()) > cap                      # something drops
    back = layer._experts(dispatch_ref(tokens, src_r.to(device), K), cap, h)
    ref, A = combine_ref(back.cpu(), topv.cpu(), slot_r)
    (ref * gout.cpu().double().reshape(-1, h)).sum().backward()
    gerr = (x.grad - x2.grad).abs().max() / x2.grad.abs().max()
    report(f"layer {device}", {"out": worst(out.reshape(-1, h), ref.detach(), (K + 1) * U * A.detach()),
                               "x.grad / 2^-16 max": float(gerr) * 2.0 ** 16})
