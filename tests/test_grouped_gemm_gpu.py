"""Ragged grouped GEMM (csrc/kernels/grouped_gemm.hip), moe_route_ragged and
MoELayer(dispatch="dropless") on the GPU.

Rule, per group and element by element (tests/gemm_ref.py): |out - ref| <=
roundings 2^-7 |ref| + K_eff 2^-24 S_eff, roundings 2 with a bias, K_eff the
contraction length (for TN the group's own row count).  Expert e's weights
carry the magnitude 2^(e % 5 - 2), so the panel of a wrong expert cannot pass.
The block tile is 128 x 128: N = 64 is half an n-tile and N = 320 leaves a
64-column last n-tile, the group sizes straddle BM = 128."""
import pytest
import torch

from paddle_amd import _ext
from paddle_amd.ops import functional as hot

from gemm_ref import check_bound, gemm_ref, scaled_rows  # noqa: E402
from moe_permute_ref import combine_ref, dispatch_ref, rnd, row_bound, worst  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = {"nn": 0, "nt": 1, "tn": 2}
# (group sizes, rows of invalid ids after the last group)
SPLITS = [([0, 1, 127, 128, 129, 0, 300, 5], 0), ([256], 0), ([0, 0, 64], 0),
          ([700, 0, 3], 13)]


def _offsets(sizes):
    return torch.tensor([0] + sizes, dtype=torch.int32).cumsum(0).to(torch.int32)


def _operands(form, sizes, tail, d0, n, seed=0):
    """CPU bf16 (a, b, bias): a [R, d0]; b [R, n] (tn), [E, d0, n] (nn) or
    [E, n, d0] (nt); bias [E, n] for nn."""
    gen = torch.Generator().manual_seed(seed)
    E, R = len(sizes), sum(sizes) + tail
    a = scaled_rows(R, d0, gen)
    if form == "tn":
        return a, scaled_rows(R, n, gen), None
    b = scaled_rows(d0 if form == "nn" else n, n if form == "nn" else d0, gen, batch=E)
    b = (b.float() * torch.exp2(torch.arange(E) % 5 - 2.0)[:, None, None]).to(torch.bfloat16)
    return a, b, scaled_rows(E, n, gen) if form == "nn" else None


def _check(form, out, a, b, bias, off, tag):
    out, E = out.cpu(), len(off) - 1
    for e in range(E):
        lo, hi = off[e], off[e + 1]
        if form == "tn":
            if hi == lo:
                assert bool((out[e] == 0).all()), f"{tag}: empty group {e}"
                continue
            ref, S, K, extra, r = gemm_ref(a[lo:hi], b[lo:hi], "tn")
            check_bound(out[e], ref, S, K, extra, r, tag=f"{tag} group {e}")
        elif hi > lo:
            ref, S, K, extra, r = gemm_ref(a[lo:hi], b[e], form,
                                           bias=None if bias is None else bias[e])
            check_bound(out[lo:hi], ref, S, K, extra, r, tag=f"{tag} group {e}")
    if form != "tn":
        assert bool((out[off[E]:] == 0).all()), f"{tag}: tail rows"


def _run(form, a, b, offsets, bias=None):
    C = _ext.get_ext()
    plan = None if form == "tn" else C.grouped_gemm_plan(offsets, a.shape[0])
    return C.grouped_gemm_bf16(a, b, offsets, plan, FORMS[form], bias)


@pytest.mark.parametrize("d0,n", [(64, 64), (192, 320)])
@pytest.mark.parametrize("sizes,tail", SPLITS)
@pytest.mark.parametrize("form", list(FORMS))
def test_forms_meet_bound(form, sizes, tail, d0, n):
    a, b, bias = _operands(form, sizes, tail, d0, n)
    off = _offsets(sizes)
    ag, bg, og = a.cuda(), b.cuda(), off.cuda()
    biasg = None if bias is None else bias.cuda()
    out = _run(form, ag, bg, og, biasg)
    _check(form, out, a, b, bias, off.tolist(), f"grouped {form} {sizes}+{tail} {d0}x{n}")
    assert torch.equal(out, _run(form, ag, bg, og, biasg))
    # the rows of invalid ids take no part
    ag[int(off[-1]):] = float("nan")
    if form == "tn":
        bg[int(off[-1]):] = float("nan")
    assert torch.equal(out, _run(form, ag, bg, og, biasg))


def test_graph_replay_follows_new_offsets():
    """Plan + NN captured once; the offsets are rewritten in place to another
    split of the same rows, so a host read at capture would show."""
    sizes, d0, n = [100, 0, 200, 84], 128, 192
    a, b, bias = _operands("nn", sizes, 0, d0, n)
    ag, bg, biasg, og = a.cuda(), b.cuda(), bias.cuda(), _offsets(sizes).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run("nn", ag, bg, og, biasg)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _run("nn", ag, bg, og, biasg)
    for split in ([3, 253, 128, 0], [0, 0, 0, 384], [129, 127, 64, 51]):
        og.copy_(_offsets(split))
        graph.replay()
        torch.cuda.synchronize()
        _check("nn", out, a, b, bias, _offsets(split).tolist(), f"graph {split}")
        assert torch.equal(out, _run("nn", ag, bg, og, biasg))


def _args(form="nn"):
    a, b, bias = _operands(form, [70, 58], 0, 64, 128)
    off = _offsets([70, 58]).cuda()
    return {"a": a.cuda(), "b": b.cuda(), "offsets": off, "bias": bias.cuda(),
            "tile_map": _ext.get_ext().grouped_gemm_plan(off, 128)}


REFUSALS = [
    ("a", lambda k: k.update(a=k["a"].float())),
    ("a", lambda k: k.update(a=k["a"][:, ::2])),
    ("a", lambda k: k.update(a=torch.cat([k["a"].reshape(-1), k["a"].reshape(-1)])[4:4 + 128 * 64].view(128, 64))),
    (r"a columns \(K\)", lambda k: k.update(a=k["a"][:, :32].contiguous(), b=k["b"][:, :32].contiguous())),
    ("b", lambda k: k.update(b=k["b"].cpu())),
    ("b", lambda k: k.update(b=k["b"][:1])),
    (r"b columns \(N\)", lambda k: k.update(b=k["b"][:, :, :96].contiguous(), bias=None)),
    ("offsets", lambda k: k.update(offsets=k["offsets"].long())),
    ("offsets", lambda k: k.update(offsets=torch.zeros(1026, dtype=torch.int32, device="cuda"))),
    ("tile_map", lambda k: k.update(tile_map=None)),
    ("tile_map", lambda k: k.update(tile_map=k["tile_map"][:-1])),
    ("bias", lambda k: k.update(bias=k["bias"][:, :64])),
    ("bias", lambda k: k.update(form=1, b=k["b"].transpose(1, 2).contiguous())),
]


@pytest.mark.parametrize("operand,spoil", REFUSALS)
def test_contract_refusals(operand, spoil):
    kw = dict(_args(), form=0)
    spoil(kw)
    with pytest.raises(RuntimeError, match=f"grouped_gemm_bf16: {operand} "):
        _ext.get_ext().grouped_gemm_bf16(**kw)


def _topi(T, K, E, bad=False):
    g = torch.Generator().manual_seed(T)
    topi = torch.rand(T, E, generator=g).argsort(1)[:, :K].to(torch.int32)
    if bad:
        topi[::7, 0] = E
        topi[3::11, K - 1] = -1
    return topi.contiguous()


@pytest.mark.parametrize("T,K,E,bad", [(150, 2, 4, False), (65, 1, 64, False),
                                       (130, 4, 8, False), (1, 2, 4, False),
                                       (150, 2, 4, True), (5000, 2, 8, True)])
def test_route_ragged_and_row_movers(T, K, E, bad):
    """The maps equal the torch spec exactly; the existing row movers serve
    the compact layout (slots = T * K) inside the bounds of moe_permute_ref."""
    topi = _topi(T, K, E, bad)
    want = hot.moe_route_ragged(topi, E)                   # CPU: the spec
    got = hot.moe_route_ragged(topi.cuda(), E)
    for g, w in zip(got, want):
        assert g.dtype == torch.int32 and torch.equal(g.cpu(), w)
    slot_of, src_of, offsets = got
    assert int(offsets[E]) == int((slot_of >= 0).sum()) == int((src_of >= 0).sum())
    h = 64
    x, w = rnd((T, h), torch.bfloat16, "cuda", 1), torch.rand(T, K, device="cuda")
    xe = hot.moe_dispatch(x, src_of, slot_of)
    assert torch.equal(xe.cpu(), dispatch_ref(x.cpu(), want[1], K))
    out = hot.moe_combine(xe, w, slot_of, src_of)
    ref, A = combine_ref(xe.cpu(), w.cpu(), want[0])
    assert worst(out, ref, row_bound(ref, A, K, torch.bfloat16)) <= 1.0


def test_dropless_layer_bf16():
    """The bf16 layer's output, x.grad and every expert parameter's grad
    against fp64 autograd of the definition, with the layer's own topi held
    fixed and topv = the fp64 softmax of the same logits (the native fp32 gate
    is within rel = (2 (h + 1) max_e |x||wg| + 64) 2^-24 of it, relative:
    its logits are an fp32 sum of h terms).  The bounds compose the GEMM rule, first order,
    through each stored bf16 tensor, per entry (t, kk) with expert e (u = 2^-7,
    U = 2^-24, b_q the bound of q, |gelu'| <= 1.13, |gelu''| <= 0.8):
      z   2u|z| + h U (|x||w1| + |b1|)
      g   1.13 b_z + u(|g| + 1.13 b_z) + 2 GELU_POLY_ERR
      y   b_g|w2| + 2u(|y| + b_g|w2|) + I U ((|g| + b_g)|w2| + |b2|)
      out sum_kk w b_y + one rounding + the combine bound of moe_permute_ref
      dy  (u + rel)|dy|                                  (w * dout, one rounding)
      dg  b_dy|w2|^T + u(|dg| + ..) + h U (|dy| + b_dy)|w2|^T
      dz  e = 1.13 b_dg + (|dg| + b_dg)(0.8 b_z + 2 DGELU_POLY_ERR); e + (u + 4U)(|dz| + e)
      dxe b_dz|w1|^T + u(|dxe| + ..) + I U (|dz| + b_dz)|w1|^T
      dw2, db2, dw1, db1 of expert e: the summed operand errors of its rows,
          one rounding, and K_eff U sum|terms| with K_eff the group's row count
      x.grad = A + B, one more rounding: A = sum_kk dxe (unweighted combine),
          B the gate path, fp32 from dw[t, kk] = <y, dout> (error <b_y, |dout|> +
          h U <|y| + b_y, |dout|>) through |softmax Jacobian| |wg|^T, one rounding."""
    import paddle_amd as paddle
    from gemm_ref import DGELU_POLY_ERR, GELU_POLY_ERR, gelu64, gelu_grad64
    from paddle_amd.models.moe import MoELayer
    paddle.seed(0)
    E, K, h, I, T = 4, 2, 64, 128, 200
    layer = MoELayer(h, I, E, k=K, capacity_factor=0.5, dispatch="dropless")
    with torch.no_grad():
        layer.gate.wg.weight.mul_(5.0)
        layer.gate.wg.weight[0] = torch.tensor([2.0, 0.0, 0.0, -2.0])
        for b in (layer.experts.b1, layer.experts.b2):
            b.normal_(0.0, 0.1)
    layer = layer.to(device="cuda", dtype=torch.bfloat16)
    x = rnd((1, T, h), torch.bfloat16, "cpu", 1) * 0.5
    x[..., 0] = 4.0
    x = x.cuda().requires_grad_()
    gout = rnd((T, h), torch.bfloat16, "cpu", 2).double()      # exact as bf16 dout
    out = layer(x)
    (out.float() * gout.float().cuda().view(1, T, h)).sum().backward()

    tokens = x.detach().reshape(T, h)
    with torch.no_grad():
        topv, topi, _ = layer.gate(tokens)
    topi = topi.cpu()
    counts = torch.bincount(topi.reshape(-1), minlength=E)
    assert int(counts[E - 1]) == 0 and int(counts[0]) > int(0.5 * T * K / E) + 1
    ex, names = layer.experts, ("w1", "b1", "w2", "b2")
    P = [getattr(ex, n).detach().cpu().double().requires_grad_() for n in names]
    xd = tokens.cpu().double().requires_grad_()
    wg = layer.gate.wg.weight.detach().cpu().double()
    probs = torch.softmax(xd @ wg, -1)
    tv = probs.gather(1, topi)
    # the native gate's logits are an fp32 sum of h terms: softmax moves by 2 max|dlogit|
    rel = (2 * (h + 1) * (xd.detach().abs() @ wg.abs()).max(1).values + 64)[:, None] * 2.0 ** -24
    assert bool(((tv.detach() - topv.cpu().double()).abs() <= rel * tv.detach()).all())
    mm = lambda a, w: torch.einsum("ti,tij->tj", a, w)  # noqa: E731
    ref, entries = 0, []
    for kk in range(K):
        e = topi[:, kk]
        z = mm(xd, P[0][e]) + P[1][e]
        g = gelu64(z)
        y = mm(g, P[2][e]) + P[3][e]
        ref = ref + tv[:, kk, None] * y
        entries.append((e, z.detach(), g.detach(), y.detach()))
    (ref * gout).sum().backward()

    u, U = 2.0 ** -7, 2.0 ** -24
    w1, b1, w2, b2 = (p.detach() for p in P)
    xa, ga, tv, pd = xd.detach().abs(), gout.abs(), tv.detach(), probs.detach()
    zero = torch.zeros(T, h, dtype=torch.float64)
    b_out, a_out, dx_a, b_a, abs_a = zero, zero, zero, zero, zero
    b_dw, dw_abs = [], []
    err = {n: torch.zeros_like(p) for n, p in zip(names, P)}
    mag = {n: torch.zeros_like(p) for n, p in zip(names, P)}

    def add(name, e, err_rows, mag_rows):
        err[name].index_add_(0, e, err_rows)
        mag[name].index_add_(0, e, mag_rows)

    for kk, (e, z, g, y) in enumerate(entries):
        w, W1, W2 = tv[:, kk, None], w1[e].abs(), w2[e].abs()
        W1t, W2t = W1.transpose(1, 2), W2.transpose(1, 2)
        bz = 2 * u * z.abs() + h * U * (mm(xa, W1) + b1[e].abs())
        bg = 1.13 * bz + u * (g.abs() + 1.13 * bz) + 2 * GELU_POLY_ERR
        eg = mm(bg, W2)
        by = eg + 2 * u * (y.abs() + eg) + I * U * (mm(g.abs() + bg, W2) + b2[e].abs())
        b_out, a_out = b_out + w * by, a_out + w * (y.abs() + by)
        dy = w * gout
        bdy = (u + rel) * dy.abs()
        dg, edg = mm(dy, w2[e].transpose(1, 2)), mm(bdy, W2t)
        bdg = edg + u * (dg.abs() + edg) + h * U * mm(dy.abs() + bdy, W2t)
        dz = dg * gelu_grad64(z)
        edz = 1.13 * bdg + (dg.abs() + bdg) * (0.8 * bz + 2 * DGELU_POLY_ERR)
        bdz = edz + (u + 4 * U) * (dz.abs() + edz)
        dxe, edx = mm(dz, w1[e].transpose(1, 2)), mm(bdz, W1t)
        bdx = edx + u * (dxe.abs() + edx) + I * U * mm(dz.abs() + bdz, W1t)
        dx_a, b_a, abs_a = dx_a + dxe, b_a + bdx, abs_a + dxe.abs() + bdx
        b_dw.append((by * ga).sum(1) + h * U * ((y.abs() + by) * ga).sum(1))
        dw_abs.append((y * gout).sum(1).abs())
        dya, dza = dy.abs() + bdy, dz.abs() + bdz
        outer = lambda a, b: a[:, :, None] * b[:, None, :]  # noqa: E731
        add("w2", e, outer(bg, dya) + outer(g.abs(), bdy), outer(g.abs() + bg, dya))
        add("b2", e, bdy, dya)
        add("w1", e, outer(xa, bdz), outer(xa, dza))
        add("b1", e, bdz, dza)

    figs = {"out": worst(out.reshape(T, h), ref.detach(),
                         b_out + u * b_out + row_bound(ref.detach(), a_out, K, torch.bfloat16))}
    for n, p in zip(names, P):
        cnt = counts.double().view(E, *([1] * (p.dim() - 1)))
        figs[n] = worst(getattr(ex, n).grad, p.grad,
                        err[n] + u * (p.grad.abs() + err[n]) + cnt * U * mag[n])
    bound_a = b_a + u * (dx_a.abs() + b_a) + (K + 1) * U * abs_a
    jac = (tv[:, :, None] * ((torch.arange(E) == topi[:, :, None]).double() - pd[:, None, :])).abs()
    edl = (torch.stack(b_dw, 1)[:, :, None] * jac).sum(1)
    dla = (torch.stack(dw_abs, 1)[:, :, None] * jac).sum(1) + edl
    eb = edl @ wg.abs().t() + ((E + h + 8) * U + 2 * rel) * (dla @ wg.abs().t())
    bound_b = eb + u * ((xd.grad - dx_a).abs() + eb)
    figs["x.grad"] = worst(x.grad.reshape(T, h), xd.grad,
                           bound_a + bound_b + u * (xd.grad.abs() + bound_a + bound_b))
    print("dropless layer bf16 worst err/bound " + " ".join(f"{k} {v:.3f}" for k, v in figs.items()))
    assert all(v <= 1.0 for v in figs.values()), figs
    for p in ex.parameters():
        assert bool((p.grad[E - 1] == 0).all()) and bool((p.grad[0] != 0).any())


