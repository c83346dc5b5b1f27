r"""The attention backward cases (``attention_bwd_cases.py``) meet the conditions the GPU test relies on -- checked on the CPU."""

import pytest
import torch

import attention_bwd_cases as cases


def test_case_list_covers_the_kernel_paths():
    dims = {v[0] for v in cases.CASES.values()}
    toks = {v[1] for v in cases.CASES.values()}
    kinds = {v[2] for v in cases.CASES.values()}
    assert dims == {16, 32, 64, 128} and toks == {9, 70, 130}
    assert kinds == {None, "causal", "batch", "head", "tile", "wave"}


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_case_conditions(name):
    c = cases.make_case(name)
    m = c["mask"]
    if m is not None:
        assert m.any(dim=-1).all(), "a query row without a live key is outside the contract"
    (out, dq, dk, dv), e_ref = cases.reference(name)
    for g in (out, dq, dk, dv):
        assert torch.isfinite(g).all() and g.abs().max() > 0
    print(name, "e_ref (dq, dk, dv):", e_ref)
    # the GPU bound is max(4 e_ref, 1e-4): the oracle's own fp32 error stays under the floor
    assert max(e_ref) < 2.5e-5


def test_mask_strides_and_blank_tiles():
    assert cases.make_case("batch_mask_d64_l70")["mask"].shape == (cases.B, 1, 70, 70)
    assert cases.make_case("head_mask_d16_l130")["mask"].shape == (1, cases.H, 130, 130)
    m = cases.make_case("tile_mask_d64_l130")["mask"]
    assert not m[0, :64].any() and m[0, 64:].all()  # blank tile BEFORE the first live key
    assert m[1, :64].all() and not m[1, 64:128].any() and m[1, 128:].all()  # ... and AFTER it
    assert m[2].all()
    w = cases.make_case("wave_mask_d32_l70")["mask"]  # 32 x 32 tiles of the kernels' waves without a live pair
    assert not w[32:64, :32].any() and not w[:32, 32:64].any() and w[32:64, 32:].all() and w[:32, :32].all() and w[64:].all()


def test_large_logits_move_their_row_maxima_between_key_tiles():
    s = cases.logits("logits30_d64_l130")
    assert s.max() > 25 and s.min() < -25
    tiles = s.argmax(dim=-1) // 64
    assert set(tiles.unique().tolist()) == {0, 1, 2}
    # ... and the running maximum of a row changes after its first tile for many rows
    first = s[..., :64].amax(dim=-1)
    assert (s.amax(dim=-1) > first).float().mean() > 0.3
