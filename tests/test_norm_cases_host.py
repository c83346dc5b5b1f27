r"""tests/norm_cases.py on the CPU: every input family has the property it is named for, the case lists of test_gpu_norm.py reach
every branch of the launch rules they are meant for (asserted by name), M_REF is what the fp32 restatement gives, torch's own fp32
group_norm meets the device bound, and restatements with a planted fault do not."""

import functools

import pytest
import torch

import norm_cases as nc

torch.set_grad_enabled(False)


def stats(x, groups):
    xg = x.double().reshape(x.shape[0], groups, -1)
    return xg.mean(-1), xg.var(-1, unbiased=False).sqrt()


# ------------------------------------------------------------------------------------------------ the families
@pytest.mark.parametrize("name,m", [("offset10", 10), ("offset1e2", 100), ("offset1e3", 1000), ("offset1e4", 10000)])
def test_offset_families_have_their_mean_to_std_ratio(name, m):
    mean, std = stats(nc.family(name, 2, 32, 256, 8), 8)
    assert ((mean / std) > 0.8 * m).all() and ((mean / std) < 1.25 * m).all()


def test_tight_and_scaled_families():
    mean, std = stats(nc.family("tight", 2, 32, 256, 8), 8)
    assert ((mean / std) > 0.8e5).all()
    for name, s in (("scaled1e4", 1e4), ("scaled1e-3", 1e-3)):
        mean, std = stats(nc.family(name, 2, 32, 256, 8), 8)
        assert ((std / s) > 0.9).all() and ((std / s) < 1.1).all()
    assert (stats(nc.family("scaled1e-3", 2, 32, 256, 8), 8)[1] ** 2 < 0.2 * nc.EPS).all()  # variance below eps


@pytest.mark.parametrize("shape", [(2, 32, 256, 8), (30, 1000, 1, 1), (1, 10, 63, 2)])
def test_constant_group_has_variance_exactly_zero_in_fp32(shape):
    x = nc.family("constant_group", *shape)
    xg = x.reshape(shape[0] * shape[3], -1)
    const = [(r == r[0]).all().item() for r in xg]
    assert sum(const) == 2 and sorted(xg[i, 0].item() for i, c in enumerate(const) if c) == [3.25, torch.tensor(1000.1).item()]
    assert all(xg[i].double().var(unbiased=False).item() == 0.0 for i, c in enumerate(const) if c)  # (every value the same fp32 number)
    assert float(torch.tensor(1000.1)) != 1000.1  # (not exact in fp32: a mean that is summed, not copied, must still return it)


def test_zero_channel_steps_ramp_and_spikes():
    assert not nc.family("zero_row", 30, 64, 1, 1).any()
    x = nc.family("channel_steps", 1, 64, 400, 2).double()
    assert ((x.mean(-1)[0] - 10.0 * torch.arange(64)).abs() < 0.3).all()
    x = nc.family("ramp", 1, 8, 4096, 2).double()
    parts = x.reshape(1, 8, 16, 256).mean((1, 3))[0]  # chunk means 12.5 apart, each chunk's std ~ 3.7
    assert ((parts[1:] - parts[:-1]) > 11.0).all() and parts[-1] - parts[0] > 180.0
    x = nc.family("spike", 2, 32, 256, 8).reshape(2, 8, -1)
    assert ((x == nc.SPIKE).sum(-1) == 1).all()
    assert len({int(i) for i in (x == nc.SPIKE).double().argmax(-1).flatten()}) > 8  # at a random place
    x = nc.family("spike", 30, 1000, 1, 1).reshape(30, -1)
    assert ((x == nc.SPIKE).sum(-1) == 1).all()


@pytest.mark.parametrize("shape", nc.SMALL_SHAPES + nc.LARGE_SHAPES[:1] + nc.LARGE_SHAPES[3:])
def test_pivot_spike_sits_on_the_pivots_the_predictors_name(shape):
    B, C, H, W, groups, cs = shape
    HW = H * W
    px = nc.gn_pivot_pixels(HW, C, cs, groups)
    ranges = nc.gn_chunk_ranges(HW, nc.gn_nchunks(HW, cs))
    assert 0 in px and all(p0 in px for p0, p1 in ranges if p1 > p0)  # pixel 0 and the first pixel of every chunk that has one
    x = nc.gn_inputs(nc.GNCase("pivot_spike", B, C, H, W, groups, cs, 0, 0, 0, 0, 0, None))["x"]
    assert (x[:, :, px] == nc.SPIKE).all() and (x == nc.SPIKE).sum().item() == B * C * len(px)
    path, qs = nc.gn_stats_path(C, cs, groups)
    # every statistics thread that reads anything starts on a spike: its first pixel is p0 + lane, lane < the lanes per chunk
    lanes = 256 // qs if path == "vector" else -(-256 // (C // groups))
    assert all(p0 + l in px for p0, p1 in ranges for l in range(lanes) if p0 + l < p1)


# ------------------------------------------------------------------------------------------------ the branches the cases reach
def gn_fp32():
    return [c for c in nc.GN_CASES if c.half is None]


def test_groupnorm_cases_reach_the_statistics_branches():
    paths = {(nc.gn_stats_path(c.C, c.cs, c.groups), c.C != c.cs) for c in gn_fp32()}
    reached = {
        "vector, qs = 256": (("vector", 256), False) in paths,
        "vector, qs = 192": (("vector", 192), False) in paths,
        "vector, qs = 160": (("vector", 160), False) in paths,
        "vector, one padded slice": any(p[0] == "vector" and padded for p, padded in paths),
        "generic": any(p[0] == "generic" for p, _ in paths),
        "generic, padded": any(p[0] == "generic" and padded for p, padded in paths),
        "generic, narrow slices of a wide tensor": any(
            nc.gn_stats_path(c.C, c.cs, c.groups)[0] == "generic" and (c.C // c.groups) % 4 == 0 for c in gn_fp32()),
        "two sources": any(c.c1 for c in gn_fp32()),
        "Cg > 64": any(c.C // c.groups > 64 for c in gn_fp32()),
    }
    rag = [nc.gn_chunks_ragged_or_empty(c.H * c.W, nc.gn_nchunks(c.H * c.W, c.cs)) for c in gn_fp32()]
    reached["ragged chunk"] = any(r for r, _ in rag)
    reached["empty chunk"] = any(e for _, e in rag)
    items = {nc.finalize_branch(nc.finalize_items(nc.gn_nchunks(c.H * c.W, c.cs))) for c in gn_fp32()}
    for br in ("le64", "le256", "gt256"):
        reached["separate pass, finalize items " + br] = br in items
    assert (1, 12, 9, 7, 3, 16) in nc.SMALL_SHAPES and nc.gn_stats_path(12, 16, 3) == ("vector", 4)
    assert nc.gn_stats_path(12, 12, 3) == ("vector", 3)  # (1, 12, 9, 7) in 3 groups is a vector case on either stride
    assert nc.gn_nchunks(200 * 200, 64) == 156 and nc.gn_nchunks(256 * 256, 64) == 256 and nc.gn_nchunks(256 * 256, 128) == 512
    print("reached:", ", ".join(reached))
    assert all(reached.values()), [k for k, v in reached.items() if not v]
    for fam in nc.LARGE_FAMILIES:  # the large maps run at least these
        assert all(any(c.family == fam and (c.B, c.C, c.H, c.W, c.groups, c.cs) == s for c in gn_fp32()) for s in nc.LARGE_SHAPES)
    for s in nc.SMALL_SHAPES:
        assert {c.family for c in gn_fp32() if (c.B, c.C, c.H, c.W, c.groups, c.cs) == s and not c.pool} >= set(nc.FAMILIES)
    assert {(c.pool, bool(c.c1), c.act) for c in gn_fp32() if c.pool} == {(p, t, a) for p in (1, 2) for t in (False, True) for a in (0, 1)}
    assert {(c.affine, c.mod) for c in gn_fp32()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(c.half, c.family) for c in nc.GN_CASES if c.half} == {(h, f) for h in nc.HALF_ULP for f in nc.HALF_GN_FAMILIES}


def test_producer_cases_reach_the_fused_finalize_branches():
    """The fused layout's item counts of test_gpu_norm.PRODUCERS (8 groups: Cout / 32 quads per group), from the producers' rules."""
    table = {"stem": ("stem", 24, 40, 128), "wino": ("wino", 32, 16, 128), "splitk_direct": ("combine", 8, 8, 128),
             "splitk_wino": ("combine", 16, 16, 256), "wino_128items": ("wino", 64, 64, 256), "wino_512items": ("wino", 128, 128, 256)}
    items = {k: nc.finalize_items(nc.fused_chunks(kind, H, W, cout), cout // 32) for k, (kind, H, W, cout) in table.items()}
    assert items == {"stem": 24, "wino": 8, "splitk_direct": 16, "splitk_wino": 256, "wino_128items": 128, "wino_512items": 512}
    assert {nc.finalize_branch(i) for i in items.values()} == {"le64", "le256", "gt256"}


def test_rownorm_cases_reach_every_form():
    f32 = [c for c in nc.ROW_CASES if c.half is None]
    form = lambda c: nc.rownorm_path(c.C, c.cs, aligned=c.mod != 2)  # noqa: E731
    reached = {
        "register form at C = 2048": any(c.C == 2048 and form(c) == "register" for c in f32),
        "looping vector form at C = 2052": any(c.C == 2052 and form(c) == "loop_vector" for c in f32),
        "looping vector form at C = 4096": any(c.C == 4096 and form(c) == "loop_vector" for c in f32),
        "looping vector form, aligned width, misaligned modulation": any(
            nc.rownorm_path(c.C, c.cs) == "register" and form(c) == "loop_vector" for c in f32),
        "scalar form with cs > C": any(form(c) == "scalar" and c.cs > c.C for c in f32),
        "rows > 16384, rows_per_batch not dividing the wave count": any(
            c.B * c.rpb > 16384 and nc.rownorm_waves(c.B * c.rpb) % c.rpb != 0 and c.mod for c in f32),
        "weight on and off": {c.weight for c in f32} == {0, 1},
        "modulation on, off, misaligned": {c.mod for c in f32} == {0, 1, 2},
        "2-byte at C = 8": any(c.half and c.C == 8 for c in nc.ROW_CASES),
        "2-byte at C = 4096": any(c.half and c.C == 4096 for c in nc.ROW_CASES),
    }
    print("reached:", ", ".join(reached))
    assert all(reached.values()), [k for k, v in reached.items() if not v]
    assert {c.C for c in f32} >= set(nc.ROW_WIDTHS) and {c.C for c in nc.ROW_CASES if c.half} >= set(nc.ROW_WIDTHS_HALF)
    assert all(nc.rownorm_h16_ok(c.C, c.cs, 2 * c.cs + 4) for c in nc.ROW_CASES if c.half)
    assert not nc.rownorm_h16_ok(12, 16) and not nc.rownorm_h16_ok(4104, 4104) and nc.rownorm_waves(18000) == 16384
    for kind in (0, 1):
        for C in nc.ROW_WIDTHS:
            assert {c.family for c in f32 if c.C == C and c.kind == kind} >= set(nc.ROW_FAMILIES)
    assert {(c.kind, c.half) for c in nc.ROW_CASES} == {(k, h) for k in (0, 1) for h in (None, *nc.HALF_ULP)}


# ------------------------------------------------------------------------------------------------ the bound
@functools.lru_cache(maxsize=None)
def restatement_ratios():
    r"""(worst ratio of the fp32 restatement, of torch's fp32 group_norm) over the GPU test's cases."""
    worst, worst_torch = 0.0, 0.0
    for c in nc.GN_CASES:
        inp = nc.gn_inputs(c)
        kw = nc.gn_kwargs(c, inp)
        ref, unit = nc.groupnorm_ref(inp["x"], **kw)
        worst = max(worst, nc.worst_ratio(nc.groupnorm_fp32(inp["x"], **kw), ref, unit)[0])
        worst_torch = max(worst_torch, nc.worst_ratio(nc.groupnorm_torch_fp32(inp["x"], **kw), ref, unit)[0])
    for c in nc.ROW_CASES:
        inp = nc.row_inputs(c)
        kw = dict(weight=inp["weight"], scale=inp["scale"], shift=inp["shift"], rows_per_batch=c.rpb)
        ref, unit = nc.rownorm_ref(inp["x"], c.kind, **kw)
        worst = max(worst, nc.worst_ratio(nc.rownorm_fp32(inp["x"], c.kind, **kw), ref, unit)[0])
    return worst, worst_torch


def test_m_ref_is_what_the_restatement_gives():
    worst, worst_torch = restatement_ratios()
    print(f"fp32 restatement: worst ratio {worst:.2f} (M_REF {nc.M_REF}); torch fp32 group_norm: {worst_torch:.2f} (M {nc.M_DEVICE})")
    assert worst <= nc.M_REF <= 1.25 * worst
    assert nc.M_DEVICE == 4.0 * nc.M_REF
    assert worst_torch <= nc.M_DEVICE  # a bound the reference implementation could not meet would be worthless


def faulty_gn(fault, fam, shape=(2, 64, 32, 32, 8)):
    B, C, H, W, groups = shape
    c = nc.GNCase(fam, B, C, H, W, groups, C, 0, 1, 1, 1, 0, None)
    inp = nc.gn_inputs(c)
    kw = nc.gn_kwargs(c, inp)
    ref, unit = nc.groupnorm_ref(inp["x"], **kw)
    return nc.worst_ratio(nc.groupnorm_fp32(inp["x"], fault=fault, **kw), ref, unit)[0]


def test_planted_faults_exceed_the_device_bound():
    """The check that the bound can fail: each fault passes on ``unit`` data (or nearly) and fails where its family aims."""
    naive = {f: faulty_gn("naive", f) for f in ("unit", "offset1e2", "offset1e3", "offset1e4", "tight")}
    cross = {f: faulty_gn("no_cross", f) for f in ("unit", "ramp", "offset1e3")}
    print("naive E[x^2] - E[x]^2:", {k: round(v, 1) for k, v in naive.items()})
    print("Chan merge without the cross term:", {k: round(v, 1) for k, v in cross.items()})
    assert naive["unit"] <= nc.M_DEVICE and max(naive[f] for f in ("offset1e3", "offset1e4", "tight")) > nc.M_DEVICE
    assert cross["ramp"] > nc.M_DEVICE
    biased = {}
    for C in (4, 64, 1024):
        c = nc.RowCase("unit", 0, 2, 15, C, C, 1, 1, None)
        inp = nc.row_inputs(c)
        kw = dict(weight=inp["weight"], scale=inp["scale"], shift=inp["shift"], rows_per_batch=c.rpb)
        ref, unit = nc.rownorm_ref(inp["x"], 0, **kw)
        biased[C] = nc.worst_ratio(nc.rownorm_fp32(inp["x"], 0, fault="biased", **kw), ref, unit)[0]
    print("LayerNorm dividing by C:", {k: round(v, 1) for k, v in biased.items()})
    assert min(biased.values()) > nc.M_DEVICE
