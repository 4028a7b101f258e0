"""sampling="device" in the runners on the torch path of sample_tokens: a
request's tokens do not depend on what shares its batch."""
import pytest
import torch

from paddle_amd.serving import Engine, GPTModelRunner, Request

PROMPTS = [[3, 7, 11], [5, 9, 2, 8, 1], [4, 4, 6], [10, 12, 14, 16]]
# request i: (temperature, top_p, top_k, seed); 0 and 2 are greedy
PARAMS = [(0.0, 1.0, 0, None), (0.9, 0.8, 0, 1234), (0.0, 1.0, 0, None),
          (1.3, 1.0, 5, 2**63 + 77)]


def serve(model, which, sampling, **kw):
    """Serve requests `which` of PROMPTS to completion; their out_ids."""
    dev = model.lm_head.weight.device
    runner = GPTModelRunner(model, num_blocks=64, block_size=16, device=dev,
                            max_seq=128, sampling=sampling, **kw)
    eng = Engine(runner, num_blocks=64, block_size=16, max_batch=4)
    reqs = []
    for i in which:
        t, p, k, s = PARAMS[i] if sampling == "device" else (0.0, 1.0, 0, None)
        reqs.append(Request(prompt_ids=PROMPTS[i], max_new_tokens=6,
                            temperature=t, top_p=p, top_k=k, seed=s))
        eng.add_request(reqs[-1])
    eng.run_until_done()
    assert all(r.done and len(r.out_ids) == 6 for r in reqs)
    return [r.out_ids for r in reqs]


def check_batch_independence(model, **kw):
    mixed = serve(model, range(4), "device", **kw)
    greedy = serve(model, range(4), "host", **kw)
    assert mixed[0] == greedy[0] and mixed[2] == greedy[2]
    assert mixed[1] != greedy[1] and mixed[3] != greedy[3]   # they do sample
    chunked = serve(model, range(4), "device", prefill_chunk=4, **kw)
    for i in (1, 3):
        assert serve(model, [i], "device", **kw)[0] == mixed[i], i
        assert chunked[i] == mixed[i], i


def test_device_sampling_is_batch_independent_cpu():
    import paddle_amd as paddle
    from paddle_amd.models import build_gpt
    paddle.seed(0)
    model = build_gpt("gpt3-tiny", max_seq_len=128).to("cpu").float()
    check_batch_independence(model)
    with pytest.raises(ValueError, match="sampling"):
        GPTModelRunner(model, num_blocks=4, device=torch.device("cpu"),
                       sampling="gpu")
