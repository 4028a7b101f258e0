"""fp8 vs bf16 grouped-expert FFN microbench (config-5 shapes).
--layer index|fused|dropless: one MoELayer forward+backward instead (T 8192,
h 1024, E 64, k 2, bf16) with that dispatch mode, and its peak memory;
--route: moe_route block forms."""
import sys, os, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import paddle_amd as paddle
from paddle_amd.models.moe import GroupedExperts
from paddle_amd.incubate.fp8 import _Fp8GroupedFFN

def bench(fn, iters=10):
    for _ in range(3): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / iters * 1e3

def layer_bench(mode):
    from paddle_amd.models.moe import MoELayer
    paddle.seed(0)
    layer = MoELayer(1024, 4096, 64, k=2, dispatch=mode).to(
        device="cuda", dtype=torch.bfloat16)
    x = torch.randn(8, 1024, 1024, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    def fb():
        (layer(x).float().sum() + layer.aux_loss).backward()
    ms = bench(fb, 20)
    print(f"MoELayer f+b T8192 h1024 E64 k2 dispatch={mode}: {ms:.3f} ms, "
          f"peak {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB", flush=True)

def route_bench():
    C = paddle._ext.get_ext()
    topi = torch.rand(8192, 64, device="cuda").argsort(1)[:, :2].int().contiguous()
    for waves in (1, 4, 16):
        ms = bench(lambda: C.moe_route(topi, 64, 513, block_waves=waves), 200)
        print(f"moe_route T8192 K2 E64 block_waves={waves}: {ms * 1e3:.1f} us/call",
              flush=True)

if "--layer" in sys.argv:
    layer_bench(sys.argv[sys.argv.index("--layer") + 1])
    sys.exit(0)
if "--route" in sys.argv:
    route_bench()
    sys.exit(0)

for N in (512, 1024, 2048):
    E, h, I = 64, 1024, 4096
    ge = GroupedExperts(E, h, I)
    for p in ge.parameters():
        p.data = p.data.to("cuda", torch.bfloat16)
    x = torch.randn(E, N, h, device="cuda", dtype=torch.bfloat16)
    xg = x.clone().requires_grad_(True)
    t_bf = bench(lambda: ge(x))
    print("bf16 fwd ok", flush=True)
    t_f8 = bench(lambda: _Fp8GroupedFFN.apply(x, ge.w1, ge.b1, ge.w2, ge.b2))
    print("fp8 fwd ok", flush=True)
    def bf_fb():
        ge(xg).sum().backward()
    def f8_fb():
        _Fp8GroupedFFN.apply(xg, ge.w1, ge.b1, ge.w2, ge.b2).sum().backward()
    t_bfb = bench(bf_fb)
    print("bf16 f+b ok", flush=True)
    t_f8b = bench(f8_fb)
    print("fp8 f+b ok", flush=True)
    print(f"E{E} N{N}: fwd bf16 {t_bf:6.2f}ms fp8 {t_f8:6.2f}ms | "
          f"f+b bf16 {t_bfb:6.2f}ms fp8 {t_f8b:6.2f}ms", flush=True)
    del ge, x, xg
    torch.cuda.empty_cache()
