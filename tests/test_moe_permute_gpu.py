"""moe_route (csrc/kernels/moe.hip) and the row movers of moe_permute.hip
through paddle_amd.ops.functional: integer-exact maps, bit-exact dispatch,
combine / dy / dw inside the bounds of tests/moe_permute_ref.py, autograd,
MoELayer(dispatch="fused"), graph capture and the binding contract."""
import pytest
import torch

from paddle_amd import _ext
from paddle_amd.ops import functional as hot

from moe_permute_ref import (CASES, SHAPES, check_case, check_layer,  # noqa: E402
                             combine_ref, dispatch_ref, make_topi, rnd,
                             route_ref, row_bound, worst)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,dtype,bad_token", CASES)
def test_kernels_meet_bounds(shape, dtype, bad_token):
    check_case("cuda", shape, dtype, bad_token)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[3]])
@pytest.mark.parametrize("waves", [1, 4, 16])
def test_route_block_forms_agree(shape, waves):
    T, K, E, cap, _ = shape
    topi = make_topi(T, K, E, bad_token=True)
    got = _ext.get_ext().moe_route(topi.cuda(), E, cap, block_waves=waves)
    for g, r in zip(got, route_ref(topi, E, cap)):
        assert torch.equal(g.cpu(), r)


def test_moe_layer_fused():
    check_layer("cuda")


def test_graph_replay_follows_new_inputs():
    """One capture of route + dispatch + combine; topi, x and w are rewritten
    in place before each replay, so a host read at capture would show."""
    T, K, E, cap, h = SHAPES[0]
    topi, x = make_topi(T, K, E).cuda(), rnd((T, h), torch.bfloat16, "cuda", 1)
    w = torch.rand(T, K, device="cuda")

    def run():
        slot_of, src_of, counts = hot.moe_route(topi, E, cap)
        xe = hot.moe_dispatch(x, src_of, slot_of)
        return slot_of, src_of, counts, xe, hot.moe_combine(xe, w, slot_of, src_of)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        outs = run()
    for seed in (11, 12, 13):
        topi.copy_(make_topi(T, K, E, seed=seed))
        x.copy_(rnd((T, h), torch.bfloat16, "cpu", seed))
        w.copy_(torch.rand(T, K, generator=torch.Generator().manual_seed(seed)))
        graph.replay()
        torch.cuda.synchronize()
        refs = route_ref(topi.cpu(), E, cap)
        xe = dispatch_ref(x.cpu(), refs[1], K)
        for got, ref in zip(outs[:4], refs + [xe]):
            assert torch.equal(got.cpu(), ref)
        ref, A = combine_ref(xe, w.cpu(), refs[0])
        assert worst(outs[4], ref, row_bound(ref, A, K, torch.bfloat16)) <= 1.0
        assert all(torch.equal(a, b) for a, b in zip(outs, run()))


ARGS = {"moe_route": ("topi", "E", "cap"), "moe_dispatch": ("x", "src_of", "K"),
        "moe_combine": ("y", "w", "slot_of"), "moe_combine_bwd": ("y", "x", "w", "src_of")}


def _misaligned(t):
    return torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)[4:].view(t.shape)


# (op, operand to spoil, how, what the message must say); in moe_combine_bwd
# the operand "x" is dout
REFUSALS = [
    ("moe_route", "topi", lambda t: t.cpu(), "topi must be a GPU"),
    ("moe_route", "topi", lambda t: t.repeat(1, 5), r"topi needs 1 <= K <= 8"),
    ("moe_route", "E", lambda e: 0, "num_experts must be >= 1"),
    ("moe_route", "cap", lambda c: 0, "cap must be >= 1"),
    ("moe_route", "E", lambda e: 1 << 28, r"num_experts \* cap must be < 2\^31"),
    ("moe_dispatch", "x", lambda t: t.half(), "x must be bfloat16 or float32"),
    ("moe_dispatch", "x", lambda t: t.t(), "x must be contiguous"),
    ("moe_dispatch", "x", lambda t: t[:, :12].contiguous(), "x needs h % 8 == 0"),
    ("moe_dispatch", "x", _misaligned, "x must be 16-byte aligned"),
    ("moe_dispatch", "src_of", lambda t: t.long(), "src_of must be contiguous int32"),
    ("moe_dispatch", "K", lambda k: 9, "needs 1 <= K <= 8"),
    ("moe_combine", "slot_of", lambda t: t.long(), "slot_of must be contiguous int32"),
    ("moe_combine", "w", lambda t: t.bfloat16(), r"w must be contiguous float32 \[T, K\]"),
    ("moe_combine_bwd", "y", lambda t: t[:-1], "y must have one row per src_of"),
    ("moe_combine_bwd", "x", lambda t: t.float(), "dout must have the dtype and h"),
]


@pytest.mark.parametrize("op,operand,spoil,says", REFUSALS,
                         ids=[f"{i}-{r[0]}-{r[1]}" for i, r in enumerate(REFUSALS)])
def test_contract_refusals(op, operand, spoil, says):
    C = _ext.get_ext()
    T, K, E, cap, h = 16, 2, 4, 8, 16
    a = dict(topi=make_topi(T, K, E).cuda(), E=E, cap=cap, K=K,
             x=rnd((T, h), torch.bfloat16, "cuda", 1), w=torch.rand(T, K, device="cuda"),
             y=rnd((E * cap, h), torch.bfloat16, "cuda", 2))
    a["slot_of"], a["src_of"], _ = C.moe_route(a["topi"], E, cap)
    getattr(C, op)(*[a[n] for n in ARGS[op]])            # the good call passes
    a[operand] = spoil(a[operand])
    with pytest.raises(RuntimeError, match=f"{op}: {says}"):
        getattr(C, op)(*[a[n] for n in ARGS[op]])
