"""moe_route / moe_dispatch / moe_combine off the native path: the torch
implementations of paddle_amd.ops.functional meet the bounds of
tests/moe_permute_ref.py, and the bounds reject three planted mistakes."""
import pytest
import torch

from moe_permute_ref import (CASES, SHAPES, check_case, check_layer,  # noqa: E402
                             combine_ref, dispatch_ref, make_topi, rnd,
                             route_ref, row_bound, worst)


@pytest.mark.parametrize("shape,dtype,bad_token", CASES)
def test_fallback_meets_bounds(shape, dtype, bad_token):
    check_case("cpu", shape, dtype, bad_token)


@pytest.mark.parametrize("mistake", ["restart_per_kk", "src_mod_T", "drop_last_kk"])
def test_bounds_reject_planted_mistakes(mistake):
    # the shape whose last choices are kept: in the other K > 1 shapes the
    # earlier choices fill every expert and leaving out the last kk is no change
    T, K, E, cap, h = SHAPES[1]
    topi = make_topi(T, K, E)
    slot_of, src_of, _ = route_ref(topi, E, cap)
    x, w = rnd((T, h), torch.bfloat16, "cpu", 1), torch.rand(T, K)
    ref, A = combine_ref(dispatch_ref(x, src_of, K), w, slot_of)
    bound = row_bound(ref, A, K, torch.bfloat16)
    assert worst(ref.to(torch.bfloat16), ref, bound) <= 1.0
    bad_slot, bad_src, _ = route_ref(topi, E, cap, restart_per_kk=mistake == "restart_per_kk")
    bad = combine_ref(dispatch_ref(x, bad_src, K, by_mod=mistake == "src_mod_T"), w,
                      bad_slot, drop_last=mistake == "drop_last_kk")[0]
    assert worst(bad.to(torch.bfloat16), ref, bound) == float("inf")


def test_moe_layer_fused_fallback():
    check_layer("cpu")
