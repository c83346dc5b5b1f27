"""engine.PlanCache, engine.plan_mode and engine.content_key on the host: what makes a plan stale, what is dropped, in what order."""

import pytest
import torch
from torch import nn

from azula_amd import engine
from azula_amd.engine import PlanCache, content_key, plan_mode


class Maker:
    r"""A counting ``make``: every plan is a new object."""

    def __init__(self) -> None:
        self.calls = 0

    def __call__(self) -> object:
        self.calls += 1
        return object()


@pytest.fixture
def cached():
    torch.manual_seed(0)
    return nn.Linear(4, 4), PlanCache(), Maker()


def other(value):
    r"""Another value of a switch's own type."""
    if isinstance(value, bool):
        return not value
    if isinstance(value, int):
        return value + 1
    return {"f16x2": "native", "1": "0"}.get(value, "1")


def test_repeated_get_returns_the_same_object(cached):
    module, cache, make = cached
    p = cache.get("a", make, module)
    assert cache.get("a", make, module) is p and make.calls == 1
    assert isinstance(cache, dict) and list(cache.values()) == [p]


def test_parameter_changes_rebuild_and_drop_the_old_stamp(cached):
    module, cache, make = cached
    a, b = cache.get("a", make, module), cache.get("b", make, module)
    with torch.no_grad():
        module.weight.add_(1)
    a2 = cache.get("a", make, module)
    assert a2 is not a and make.calls == 3
    assert list(cache.items()) == [("a", a2)]  # ("b" carried the old stamp: gone, not only shadowed)
    assert cache.get("b", make, module) is not b
    module.load_state_dict({k: v + 1 for k, v in module.state_dict().items()})
    a3 = cache.get("a", make, module)
    assert a3 is not a2 and list(cache) == ["a"]
    module.half()
    assert cache.get("a", make, module) is not a3
    assert cache.get("a", make, module) is cache["a"] and make.calls == 6


def test_mode_flip_rebuilds_both_ways(cached, monkeypatch):
    module, cache, make = cached
    monkeypatch.setattr(engine, "FP32_MFMA", "f16x2")
    p = cache.get("a", make, module)
    monkeypatch.setattr(engine, "FP32_MFMA", "native")
    q = cache.get("a", make, module)
    assert q is not p and cache.get("a", make, module) is q
    monkeypatch.setattr(engine, "FP32_MFMA", "f16x2")
    r = cache.get("a", make, module)
    assert r is not q and r is not p and make.calls == 3


@pytest.mark.parametrize("name", engine.PLAN_SWITCHES)
def test_every_switch_is_part_of_the_mode(name, monkeypatch):
    before = plan_mode()
    assert before == plan_mode()
    monkeypatch.setattr(engine, name, other(getattr(engine, name)))
    after = plan_mode()
    at = engine.PLAN_SWITCHES.index(name)
    assert after != before and after[:at] == before[:at] and after[at + 1 :] == before[at + 1 :]


def test_the_mode_names_every_environment_switch():
    r"""Every switch of engine.py that is read from the environment is on the list (beside those only tests assign to)."""
    listed = {"FP32_MFMA", "WINOGRAD", "WINO_X3", "F16X2_DYNAMIC", "F16X2_MOMENTS", "GN_FUSED", "HALF_ACT", "QK_PREP", "STEM_PLANAR",
              "AFFINE_FUSED", "ATTN_H2", "ATTN_X3", "WINOGRAD4_MIN_TILES"}
    assert listed <= set(engine.PLAN_SWITCHES) and len(set(engine.PLAN_SWITCHES)) == len(engine.PLAN_SWITCHES)


def test_changed_extra_rebuilds(cached):
    module, cache, make = cached
    p = cache.get("a", make, module, extra=((3, "wh2d"),))
    assert cache.get("a", make, module, extra=((3, "wh2d"),)) is p
    q = cache.get("a", make, module, extra=())
    assert q is not p and cache.get("a", make, module) is q and make.calls == 2


def test_size_bound_is_fifo(cached):
    module, cache, make = cached
    assert cache.max_live == 4
    plans = {k: cache.get(k, make, module) for k in "abcd"}
    assert cache.get("a", make, module) is plans["a"]  # (a hit: no reordering ...)
    assert list(cache) == list("abcd")
    e = cache.get("e", make, module)
    assert list(cache.items()) == [("b", plans["b"]), ("c", plans["c"]), ("d", plans["d"]), ("e", e)]  # (... so "a" is the oldest)
    assert cache.get("a", make, module) is not plans["a"] and list(cache) == list("cdea")
    cache.max_live = 6
    for k in "fg":
        cache.get(k, make, module)
    assert list(cache) == list("cdeafg")
    cache.get("h", make, module)
    assert list(cache) == list("deafgh")


def test_keys_come_back_as_passed_and_clear_empties(cached):
    module, cache, make = cached
    keys = [("vjp", 2, 16, 16, 1, "cuda:0"), (2, 1, 16, 16, 1, "cuda:0", None, 139845, 0, False), (2, 16, 1, (b"\x00\x01", None), "cuda:0")]
    plans = [cache.get(k, make, module) for k in keys]
    assert [k for k, _ in cache.items()] == keys and [p for _, p in cache.items()] == plans
    assert next(iter(cache.values())) is plans[0]
    cache.clear()
    assert len(cache) == 0 and cache.get(keys[0], make, module) is not plans[0]


class Holder(nn.Module):
    pass


def test_content_key_compares_bytes(monkeypatch):
    holder = Holder()
    pos = torch.cartesian_prod(torch.arange(4.0), torch.arange(4.0))
    mask = torch.ones(16, 16, dtype=torch.bool).tril()
    k = content_key(holder, pos, mask)
    assert content_key(holder, pos.clone(), mask.clone()) == k  # (two different tensors, equal bytes)
    moved = pos.clone()
    moved[5, 1] += 0.5
    assert content_key(holder, moved, mask) != k
    flipped = mask.clone()
    flipped[3, 9] = True
    assert content_key(holder, pos, flipped) != k
    assert content_key(holder, pos, None) != k and content_key(holder, pos, None) == content_key(holder, pos.clone(), None)
    assert content_key(holder, pos.reshape(8, 4), mask) != k  # (the shape is part of the content)

    copies = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **kw: (copies.append(1), real(t, *a, **kw))[1])
    first = content_key(holder, pos, mask)
    assert first == k and len(copies) == 2
    assert content_key(holder, pos, mask) == k and len(copies) == 2  # (the same objects again: recognised, nothing copied)
    with torch.no_grad():
        pos[0, 0] = 7.0  # (an in-place write bumps the version counter: read again)
    assert content_key(holder, pos, mask) != k and len(copies) == 4
    assert len(holder._plan_seen) <= 2
