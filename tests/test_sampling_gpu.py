"""sample_tokens HIP kernel (csrc/kernels/sampling.hip) against an fp64 /
exact-integer reference driven by explicit rand_bits."""
import pytest
import torch

from paddle_amd.ops.functional import sample_tokens

BF16, F32 = torch.bfloat16, torch.float32
ONE = 1 << 40


def reference(x, T, P, K, r):
    """x [B, V], per-row T, P, K (CPU tensors), r a list of u64 integers.
    Returns (tokens, order [B, V], kept-set sizes, fp64 kept probabilities)."""
    x = x.double()
    V = x.shape[1]
    sx, order = torch.sort(x, dim=1, descending=True, stable=True)
    Ts = torch.where(T > 0, T, torch.ones_like(T)).double()
    w = torch.round(ONE * torch.exp((x - sx[:, :1]) / Ts[:, None])).long()
    sw = w.gather(1, order)
    before = sw.cumsum(1) - sw
    thr = torch.ceil(torch.where(P < 1, P, torch.zeros_like(P)).double()
                     * sw.sum(1).double()).long()
    keep = ((P >= 1)[:, None] | (before < thr[:, None])) \
        & ((K <= 0)[:, None] | (torch.arange(V)[None] < K[:, None]))
    keep[:, 0] = True
    kw = torch.zeros_like(w).scatter(1, order, sw * keep)
    cdf = kw.cumsum(1)
    t = torch.tensor([(ri * z) >> 64 for ri, z in zip(r, cdf[:, -1].tolist())])
    tok = torch.searchsorted(cdf, t[:, None], right=True)[:, 0]
    exact = ~(T > 0) | (K == 1) | ~(P > 0)
    return (torch.where(exact, order[:, 0], tok), order, keep.sum(1),
            kw.double() / cdf[:, -1:].double())


def row_params(B):
    b = torch.arange(B)
    T = torch.tensor([0.0, 0.5, 1.0, 1.7])[b % 4]
    P = torch.tensor([1.0, 0.9, 0.3, 0.0])[(b // 4) % 4]
    K = torch.tensor([0, 1, 40], dtype=torch.int32)[(b // 16) % 3]
    return T, P, K


def u64(r):
    return [int(v) & (2**64 - 1) for v in r.tolist()]


def zeros64(B):
    return torch.zeros(B, dtype=torch.int64, device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,B,V,strided", [
    (BF16, 512, 1000, False), (BF16, 512, 9001, False), (BF16, 3, 50257, False),
    (BF16, 64, 50304, False), (BF16, 16, 70001, False), (F32, 64, 9001, False),
    (F32, 16, 40001, False), (BF16, 64, 9001, True)])
def test_reference_parity(dtype, B, V, strided):
    """Rows that differ from the fp64 reference, measured on MI355X: 0 of the
    sampled rows at every shape (docs/KERNELS.md "token sampling")."""
    g = torch.Generator().manual_seed(V + B)
    wide = (torch.randn(B, V + (37 if strided else 0), generator=g) * 3).to(dtype)
    x = wide[:, 5:5 + V] if strided else wide
    T, P, K = row_params(B)
    r = torch.randint(-2**63, 2**63 - 1, (B,), generator=g)
    xd = wide.cuda()[:, 5:5 + V] if strided else wide.cuda()
    assert xd.is_contiguous() != strided
    out = sample_tokens(xd, T.cuda(), P.cuda(), K.cuda(), zeros64(B),
                        zeros64(B), r.cuda()).cpu()
    ref, order, nkeep, _ = reference(x, T, P, K, u64(r))
    exact = ~(T > 0) | (K == 1) | ~(P > 0)
    assert torch.equal(out[exact], ref[exact])
    diff = (~exact & (out != ref)).nonzero()[:, 0].tolist()
    print(f"{dtype} B={B} V={V}: {len(diff)} of {int((~exact).sum())} "
          "sampled rows differ")
    assert len(diff) <= 0.01 * int((~exact).sum())
    for b in diff:      # a draw on a CDF boundary may fall either way
        assert out[b] in order[b, :nkeep[b] + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["top_k", "top_p"])
@pytest.mark.parametrize("V", [1000, 9001])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_ties_and_boundary_exact(dtype, V, mode):
    """37 scattered maxima, 20 kept: every weight is exactly 2^40, so an
    even grid of 20 * k draws returns each of the 20 lowest-index maxima
    exactly k times."""
    k, g = 204, torch.Generator().manual_seed(V)
    B = 20 * k
    where = torch.randperm(V, generator=g)[:37].sort().values
    row = (-100 - 10 * torch.rand(V, generator=g)).to(dtype)
    row[where] = 5.0
    x = row.cuda()[None].expand(B, V)               # row stride 0
    r = [((2 * j + 1) << 64) // (2 * B) for j in range(B)]
    r = torch.tensor([v - 2**64 if v >= 2**63 else v for v in r]).cuda()
    ones = torch.ones(B, device="cuda")
    P = ones * (1.0 if mode == "top_k" else 19.5 / 37)
    K = torch.full((B,), 20 if mode == "top_k" else 0, dtype=torch.int32,
                   device="cuda")
    out = sample_tokens(x, ones, P, K, zeros64(B), zeros64(B), r)
    tok, cnt = out.cpu().unique(return_counts=True)
    assert torch.equal(tok, where[:20])
    assert cnt.tolist() == [k] * 20


@pytest.mark.gpu
def test_philox_draws():
    """(seed, offset) reproduces; 4096 offsets of one 8-token distribution
    stay inside the binomial bound and equal the torch path's Philox; a
    captured graph follows offset += 1 on the device."""
    n = 4096
    row = torch.tensor([2.0, 0.5, 1.0, -1.0, 1.5, 0.0, -3.0, 1.0])
    x = row.to(BF16).cuda()[None].expand(n, 8)
    ones = torch.ones(n, device="cuda")
    K = torch.zeros(n, dtype=torch.int32, device="cuda")
    seed = torch.full((n,), 20240607, dtype=torch.int64, device="cuda")
    off = torch.arange(n, device="cuda")
    out = sample_tokens(x, ones, ones, K, seed, off)
    assert torch.equal(out, sample_tokens(x, ones, ones, K, seed, off))
    assert not torch.equal(out, sample_tokens(x, ones, ones, K, seed + 1, off))
    cpu = sample_tokens(x.cpu(), ones.cpu(), ones.cpu(), K.cpu(), seed.cpu(),
                        off.cpu())
    assert torch.equal(out.cpu(), cpu)
    p = reference(row[None], torch.ones(1), torch.ones(1),
                  torch.zeros(1, dtype=torch.int32), [0])[3][0]
    cnt = torch.bincount(out.cpu(), minlength=8).double()
    assert ((cnt - n * p).abs() <= 5 * (n * p * (1 - p)).sqrt()).all(), cnt

    xs = (torch.randn(8, 1000, generator=torch.Generator().manual_seed(1)) * 3
          ).to(BF16).cuda()
    T, P, Kp = (t.cuda() for t in row_params(8))
    T = T + 0.7                                     # every row samples
    sd, of = seed[:8].clone(), zeros64(8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sample_tokens(xs, T, P, Kp, sd, of)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = sample_tokens(xs, T, P, Kp, sd, of)
    seen = []
    for _ in range(4):
        of += 1
        graph.replay()
        assert torch.equal(got, sample_tokens(xs, T, P, Kp, sd, of))
        seen.append(got.clone())
    assert not all(torch.equal(seen[0], s) for s in seen[1:])


def _args(B=4, V=64):
    d = "cuda"
    return {"logits": torch.zeros(B, V, dtype=BF16, device=d),
            "temperature": torch.ones(B, device=d),
            "top_p": torch.ones(B, device=d),
            "top_k": torch.zeros(B, dtype=torch.int32, device=d),
            "seed": zeros64(B), "offset": zeros64(B), "rand_bits": zeros64(B)}


@pytest.mark.gpu
@pytest.mark.parametrize("name,bad", [
    ("logits", lambda a: a["logits"].half()),
    ("logits", lambda a: a["logits"][0]),
    ("logits", lambda a: a["logits"][:, ::2]),
    ("logits", lambda a: a["logits"].cpu()),
    ("temperature", lambda a: a["temperature"].double()),
    ("top_p", lambda a: a["top_p"][:3]),
    ("top_k", lambda a: a["top_k"].long()),
    ("seed", lambda a: a["seed"].cpu()),
    ("offset", lambda a: a["offset"].int()),
    ("rand_bits", lambda a: a["rand_bits"].repeat(2)[::2]),
])
def test_contract(name, bad):
    from paddle_amd import _ext
    a = _args()
    a[name] = bad(a)
    with pytest.raises(RuntimeError, match=f"sample_tokens: .*{name}"):
        _ext.get_ext().sample_tokens(**a)


@pytest.mark.gpu
def test_device_sampling_is_batch_independent_gpu():
    """The CPU file's comparison on the kernels, graphs on and off."""
    import paddle_amd as paddle
    from paddle_amd.models import build_gpt
    from test_sampling_cpu import check_batch_independence
    paddle.seed(0)
    model = build_gpt("gpt3-tiny", num_heads=2, max_seq_len=128).to("cuda", BF16)
    for graphs in (True, False):
        check_batch_independence(model, use_graphs=graphs)
