r"""tests/token_cases.py on the CPU: every input has the property it is named for, torch's own fp32 evaluation meets each derived
bound with room (ratio <= 0.7, so the reference alone stays inside), and a restatement with a planted fault misses the bound or
the exact comparison -- asserted per fault, by name.  Also the argument validation of the entries test_gpu_token_kernels.py runs
(addresses that are never dereferenced) and the host-side check of the grouped linear's descriptors."""

import functools

import pytest
import torch

import token_cases as tc

torch.set_grad_enabled(False)

ROOM = 0.7


def ratio(got, ref, allowed):
    return ((got.double() - ref).abs() / allowed).max().item()


# ------------------------------------------------------------------------------------------------ (a) the inputs
@pytest.mark.parametrize("in_act,out_act", tc.LIN_ACTS)
@pytest.mark.parametrize("M,N,K", tc.LIN_SHAPES)
def test_linear_inputs(M, N, K, in_act, out_act):
    x, W, b = tc.linear_inputs(M, N, K, in_act, out_act)
    ref, allowed, S = tc.linear_ref(x, W, b, in_act, out_act)
    cols = x.abs().max(0).values
    if not in_act and K >= 3:
        mags = [cols[i::3].median().item() for i in range(3)]
        assert 10 * mags[0] < mags[1] and 10 * mags[1] < mags[2]  # columns cycle 1e-3 / 1 / 1e3
        if M * (K // 3) >= 8:  # (a single draw can be small)
            assert mags[0] < 1e-2 and 0.1 < mags[1] < 10 and mags[2] > 1e2
    if in_act:
        assert x.abs().max() <= 30 and (K < 3 or cols[2::3].max() == 30)  # the large columns saturate the clamp
    pre = (tc.silu64(x) if in_act else x.double()) @ W.double().T + b.double()
    if out_act:
        assert pre.abs().max() <= 30
    # the orthogonalised row: a cancellation far below anything a bound relative to max |ref| could see
    assert b[0] == 0 and pre[0, 0].abs() <= 1e-6 * S[0, 0]
    assert (allowed > 0).all() and torch.isfinite(allowed).all()
    if not out_act:
        assert allowed[0, 0] < 1e-3 * ref.abs().max()  # ... and the bound there is absolute, not relative to the largest output


def test_linear_forms_reach_both_kernels_and_the_row_loop():
    paths = {(tc.linear_vector_path(K, K), tc.linear_vector_path(K, K + 4), tc.linear_vector_path(K, K, 1)) for _, _, K in tc.LIN_SHAPES}
    assert (True, True, False) in paths and (False, False, False) in paths
    assert any(M > 256 for M, _, _ in tc.LIN_SHAPES) and any(K % 256 for _, _, K in tc.LIN_SHAPES) and any(K > 256 for _, _, K in tc.LIN_SHAPES)
    assert {K for K, _ in tc.ONEHOT_CASES} == {3, 40, 260, 300} and {N for _, N in tc.ONEHOT_CASES} == {1, 7}
    assert len({K for K, _, _ in tc.GROUPED_GROUPS}) == 3 and sum(not hb for _, _, hb in tc.GROUPED_GROUPS) == 1
    assert all(K % 4 == 0 for K, _, _ in tc.GROUPED_GROUPS)  # (the grouped kernel has the vector form only)


@pytest.mark.parametrize("K,N", tc.ONEHOT_CASES)
def test_onehot_linear_is_exact_in_fp32(K, N):
    x, W, b = tc.onehot_inputs(K, N)
    assert (W != 0).all() and torch.equal(x, torch.eye(K))
    assert torch.equal(tc.linear_fp32(x, W, None), W.T) and torch.equal(tc.linear_fp32(x, W, b), W.T + b)
    assert not torch.equal(W.T + b, W.T)


def test_grouped_inputs_are_exact_in_any_order():
    for (K, N, has_bias), (x, W, b, want) in zip(tc.GROUPED_GROUPS, tc.grouped_inputs()):
        assert x.shape == (tc.GROUPED_M, K) and W.shape == (N, K) and (b is not None) == has_bias
        assert ((x[:3] != 0).sum(1) == 1).all() and (x[3:] == x[3:].round()).all() and (x[3:] != 0).sum() > K
        perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
        for order in (torch.arange(K), perm, torch.arange(K - 1, -1, -1)):  # sequential fp32 accumulation in three orders
            acc = torch.zeros(tc.GROUPED_M, N)
            for k in order.tolist():
                acc = acc + x[:, k : k + 1] * W[None, :, k]
            assert torch.equal(acc if b is None else acc + b, want)


def test_silu_points_and_specials():
    p = tc.silu_points(4096)
    assert p.abs().max() == 30 and abs(p.abs().min().item() - 1e-6) < 1e-12 and (p > 0).any() and (p < 0).any()
    assert all((p.abs() < 10.0 ** (d + 1)).logical_and(p.abs() >= 10.0 ** d).sum() > 200 for d in range(-6, 1))  # every decade
    sp = torch.tensor(tc.SILU_SPECIALS)
    ref = tc.silu64(sp)
    assert ref[0] == 0 and ref[1] == 0 and torch.signbit(ref[1]) and ref[2] == 90 and 0 < -ref[3] < 1e-37
    assert tc.GRID_CAP < tc.SILU_SIZES[-1] < tc.GRID_CAP + 4096


def test_swiglu_cases():
    assert {c.cout for c in tc.SWIGLU_CASES} == {1, 9, 10, 64}
    assert {c.xs - 2 * c.cout for c in tc.SWIGLU_CASES} == {0, 2, 8}
    assert all({c.ys for c in tc.SWIGLU_CASES if c.cout == co} == {co, tc.pad4(co) + 4} for co in (1, 9, 10, 64))
    big = tc.SWIGLU_LARGE
    assert tc.GRID_CAP < big.rows * big.ys < tc.GRID_CAP + 4096 and big.ys > big.cout
    for c in tc.SWIGLU_CASES:
        x = tc.swiglu_inputs(c)
        assert torch.isnan(x[:, 2 * c.cout :]).all() and torch.isfinite(x[:, : 2 * c.cout]).all()
        assert x[:, 1 : 2 * c.cout : 2].abs().max() <= 30
        assert torch.isfinite(tc.swiglu_ref(x, c.cout)[0]).all()


def test_embedding_cases():
    assert [d // 2 for d in tc.EMB_DIMS if (d // 2) & (d // 2 - 1)] == [3, 160]  # halves that are no power of two: the orders differ
    assert max(tc.EMB_T) == 1e4 and 0.0 in tc.EMB_T and tc.GRID_CAP < tc.EMB_LARGE[0] * tc.EMB_LARGE[1] // 2 < tc.GRID_CAP + 16384
    import oracle.nets as nets  # the reference's embedding in fp64 agrees with this module's reference (another route to the same values)

    t = torch.tensor(tc.EMB_T[:5], dtype=torch.float32)
    ref, allowed = tc.embedding_ref(t, 128)
    assert ((nets.jit_timestep_embedding(t.double(), 256) - ref).abs() <= allowed).all()


def test_patch_cases():
    for p in tc.PATCH_P:
        H, W = tc.patch_hw(p)
        assert H != W and H % p == 0 and W % p == 0
        for Z in tc.PATCH_Z:
            cs = tc.patch_strides(Z, p)
            assert cs[0] == Z * p * p and cs[-1] == cs[0] + 8 and tc.pad4(cs[0]) in cs
            x = torch.arange(3 * Z * H * W, dtype=torch.float32).reshape(3, Z, H, W)
            for c in cs:
                tok = tc.patchify_ref(x, p, c)
                assert (tok[..., cs[0] :] == 0).all()
                a, b, z, hp, wp = p - 1, p // 2, Z - 1, H // p - 1, 1  # one element by the definition: feature z p p + a p + b
                assert tok[2, hp * (W // p) + wp, z * p * p + a * p + b] == x[2, z, hp * p + a, wp * p + b]
                tok[..., cs[0] :] = float("nan")
                assert torch.equal(tc.unpatchify_ref(tok, Z, H, W, p), x)
    B, Z, H, W, p, cs = tc.PATCH_LARGE
    assert tc.GRID_CAP < B * Z * H * W < 2 ** 20 and tc.GRID_CAP < B * (H // p) * (W // p) * cs < 2 ** 20 and cs > Z * p * p


def test_window_cases():
    names = {c.name for c in tc.COPY_CASES}
    assert {"front", "back", "middle", "interleave_even", "interleave_odd", "strided_pick", "grid_cap"} <= names
    for c in tc.COPY_CASES:
        assert 0 <= c.dst_off and c.dst_off + c.n <= c.dst_tokens and 0 <= c.src_off and c.src_off + c.n <= c.src_tokens
    assert max(c.B for c in tc.COPY_CASES) == 40 and {c.cs for c in tc.COPY_CASES} >= {4, 24}
    big = tc.COPY_CASES[-1]
    assert tc.GRID_CAP < big.B * big.n * big.cs // 4 < tc.GRID_CAP + 16384
    fc = tc.fill_cases(24)
    assert {c.row_bstride for c in fc} == {0, 1, 2} and {c.n for c in fc} == {1, 4}
    assert {c.dst_off for c in fc if c.n == 4} == {0, 2, 5}  # both ends and the middle of 9 tokens
    row, pos = tc.fill_inputs(fc[0])
    s = tc.token_fill_sum(row, pos, fc[0])
    assert ((s.double() - (row[:, None, :24].double() + pos[None].double())) != 0).any()  # the sums do round


@pytest.mark.parametrize("dtype", list(tc.H16_DTYPES.values()))
def test_h16_inputs_hit_the_rounding_decisions(dtype):
    extra = tc.H16_EXTRA[dtype]
    row, pos, sums = tc.h16_inputs(dtype)
    s = torch.cat(list(sums.values()))
    assert len(row) % 8 == 0 and tc.same_bits((row + pos)[: len(s)], s)  # the fp32 sums ARE the special values
    for t in (row, pos, s):
        assert torch.isfinite(t).all() and ((t.abs() >= 2.0 ** -126) | (t == 0)).all()  # normal or zero
    low = lambda v: tc.bits(v).to(torch.int64) & ((1 << extra) - 1)  # noqa: E731
    kept_lsb = lambda v: (tc.bits(v).to(torch.int64) >> extra) & 1  # noqa: E731
    half = 1 << (extra - 1)
    down, up = sums["tie_to_even_down"], sums["tie_to_even_up"]
    assert (low(down) == half).all() and (kept_lsb(down) == 0).all() and (low(up) == half).all() and (kept_lsb(up) == 1).all()
    assert (low(sums["tie_plus_ulp"]) == half + 1).all() and (low(sums["tie_minus_ulp"]) == half - 1).all()
    for v in (down, up):
        assert (v > 0).any() and (v < 0).any()
    cast = lambda v: v.to(dtype).float()  # noqa: E731
    assert (cast(down).abs() < down.abs()).all() and (cast(up).abs() > up.abs()).all()  # to the even neighbour, either direction
    assert (cast(sums["tie_plus_ulp"]).abs() > sums["tie_plus_ulp"].abs()).all()
    assert (cast(sums["tie_minus_ulp"]).abs() < sums["tie_minus_ulp"].abs()).all()
    z = sums["zeros"].to(dtype)
    assert torch.signbit(z[0]) and not torch.signbit(z[1]) and (z == 0).all()
    edge = cast(sums["overflow_edge"])
    big = torch.finfo(dtype).max
    assert edge[:4].tolist() == [big, big, float("inf"), float("inf")] and edge[4:].tolist() == [-big, -big, float("-inf"), float("-inf")]
    if dtype == torch.float16:
        assert sums["overflow_edge"][0] == 65504 and sums["overflow_edge"][2] == 65520
        sub = sums["half_subnormal"]
        assert (sub.abs() <= 2.0 ** -14).all() and (sub.abs() > 2.0 ** -26).all()  # (2^-14, the smallest normal half, closes the list)
        h = cast(sub)
        assert (h == 0).any() and ((h != 0) & (h.abs() < 2.0 ** -14)).sum() > 40  # results in the subnormal range, and the tie at 2^-25 -> 0
        k = (h.double().abs() * 2.0 ** 24)
        assert (k == k.round()).all()
        tie = sub[:9].double() * 2.0 ** 24  # (k + 1/2): to the even k
        assert (cast(sub[:9]).double() * 2.0 ** 24 % 2 == 0).all() and ((cast(sub[:9]).double() * 2.0 ** 24 - tie).abs() == 0.5).all()


def test_gather_and_cfg_cases():
    idx = tc.gather_indices(tc.GATHER_TABLE_ROWS)
    assert {-5, 0, tc.GATHER_TABLE_ROWS - 1, tc.GATHER_TABLE_ROWS + 2} <= set(idx.tolist())  # -5, 0, last, last + 3
    assert set(tc.GATHER_NCOLS) == {8, 300, 1000} and max(tc.GATHER_NCOLS) > 3 * 256  # the column loop's fourth trip
    table = torch.arange(6 * 8, dtype=torch.float32).reshape(6, 8)
    assert torch.equal(tc.gather_ref(table, idx)[:4], table[[0, 0, 5, 5]])
    assert torch.equal(tc.gather_ref(table[:1], idx), table[:1].expand(len(idx), 8))  # table_rows = 1: a broadcast
    assert set(tc.CFG_GUIDANCE) == {0.0, 7.5, -1.0} and tc.CFG_SIZES[:2] == (1, 1027) and tc.CFG_SIZES[2] > tc.GRID_CAP
    pos, neg = tc.cfg_inputs(1027)
    assert pos.abs().min() < 1e-2 and pos.abs().max() > 1e2
    d = tc.cfg_ref(pos, neg, 7.5).double() - (pos.double() + 7.5 * (pos.double() - neg.double()))
    assert (d != 0).any()  # the three operations do round
    assert torch.equal(tc.cfg_ref(pos, neg, 0.0), pos) and torch.equal(tc.cfg_ref(pos, neg, -1.0), pos + -(pos - neg))


# ------------------------------------------------------------------------------------------------ (b) torch's fp32 against the bounds
def emb_rows():
    t = torch.tensor(tc.EMB_T, dtype=torch.float32)
    yield from ((t, d // 2) for d in tc.EMB_DIMS)
    yield tc.embedding_large_t(tc.EMB_LARGE[0]), tc.EMB_LARGE[1] // 2


@functools.lru_cache(maxsize=None)
def reference_ratios():
    r = {"embedding": 0.0, "linear": 0.0, "silu": 0.0, "swiglu": 0.0}
    for t, half in emb_rows():
        ref, allowed = tc.embedding_ref(t, half)
        r["embedding"] = max(r["embedding"], ratio(tc.embedding_fp32(t, half), ref, allowed))
    for M, N, K in tc.LIN_SHAPES:
        for in_act, out_act in tc.LIN_ACTS:
            x, W, b = tc.linear_inputs(M, N, K, in_act, out_act)
            ref, allowed, _ = tc.linear_ref(x, W, b, in_act, out_act)
            r["linear"] = max(r["linear"], ratio(tc.linear_fp32(x, W, b, in_act, out_act), ref, allowed))
    p = tc.silu_points(1 << 16)
    r["silu"] = ratio(torch.nn.functional.silu(p), tc.silu64(p), tc.e_silu(p))
    sp = torch.tensor(tc.SILU_SPECIALS)  # (asserted on their own: at -90 the exact result, -7.4e-38, is most of the 1e-37 a flush to -0 is allowed)
    assert ratio(torch.nn.functional.silu(sp), tc.silu64(sp), tc.e_silu(sp)) <= 1.0
    for c in tc.SWIGLU_CASES:
        x = tc.swiglu_inputs(c)
        ref, allowed = tc.swiglu_ref(x, c.cout)
        r["swiglu"] = max(r["swiglu"], ratio(tc.swiglu_fp32(x, c.cout), ref, allowed))
    return r


@pytest.mark.parametrize("bound", ["embedding", "linear", "silu", "swiglu"])
def test_torch_fp32_meets_the_bound_with_room(bound):
    r"""Measured here: embedding 0.61, linear 0.30, silu 0.41, swiglu 0.37."""
    r = reference_ratios()
    print("reference-only ratios:", {k: round(v, 3) for k, v in r.items()})
    assert 0 < r[bound] <= ROOM


# ------------------------------------------------------------------------------------------------ (c) planted faults
def linear_fault_caught(fault):
    caught = {}
    for M, N, K in tc.LIN_SHAPES:
        x, W, b = tc.linear_inputs(M, N, K, 0, 0)
        ref, allowed, _ = tc.linear_ref(x, W, b, 0, 0)
        caught[f"fp64 {M}x{N}x{K}"] = ratio(tc.linear_fp32(x, W, b, fault=fault), ref, allowed) > 1
    for K, N in tc.ONEHOT_CASES:
        x, W, b = tc.onehot_inputs(K, N)
        caught[f"onehot K={K} N={N}"] = not torch.equal(tc.linear_fp32(x, W, None, fault=fault), W.T)
    return caught


def planted_faults():
    r"""name -> {case: caught}."""
    out = {f: linear_fault_caught(f) for f in ("last k-quad dropped", "one k counted twice")}
    for fault in ("exponent in the other order", "cos and sin swapped"):
        out[fault] = {}
        for t, half in emb_rows():
            ref, allowed = tc.embedding_ref(t, half)
            out[fault][f"half={half} rows={len(t)}"] = ratio(tc.embedding_fp32(t, half, fault=fault), ref, allowed) > 1
    out["truncating 2-byte store"] = {}
    for dtype in tc.H16_DTYPES.values():
        row, pos, sums = tc.h16_inputs(dtype)
        for name, s in sums.items():
            out["truncating 2-byte store"][f"{dtype} {name}"] = not tc.same_bits(tc.truncate_to(s, dtype), s.to(dtype))
    out["pad lanes unwritten"] = {}
    for p in tc.PATCH_P:
        H, W = tc.patch_hw(p)
        x = torch.randn(1, 3, H, W)
        for cs in tc.patch_strides(3, p):
            bad = tc.patchify_ref(x, p, cs, prefill=float("nan"), fault="pad lanes unwritten")
            out["pad lanes unwritten"][f"p={p} cs={cs}"] = not tc.same_bits(bad, tc.patchify_ref(x, p, cs))
    out["index clamp missing"] = {}
    for rows in (tc.GATHER_TABLE_ROWS, 1):
        table = torch.randn(rows, 8)
        idx = tc.gather_indices(rows)
        for i in idx.tolist():
            one = torch.tensor([i])
            out["index clamp missing"][f"rows={rows} idx={i}"] = not torch.equal(tc.gather_ref(table, one, fault="index clamp missing"),
                                                                                 tc.gather_ref(table, one))
    return out


@pytest.mark.parametrize("fault", tc.PLANTED_FAULTS)
def test_planted_fault_is_caught(fault):
    caught = planted_faults()[fault]
    print(fault, "-> caught by", [k for k, v in caught.items() if v], "; passes", [k for k, v in caught.items() if not v])
    assert any(caught.values()), fault


def test_planted_faults_are_caught_where_they_should_be():
    r"""Beyond 'somewhere': the cases each fault is aimed at."""
    pf = planted_faults()
    assert set(pf) == set(tc.PLANTED_FAULTS)
    assert all(pf["last k-quad dropped"].values()) and all(pf["one k counted twice"].values())  # every linear case sees a lost or doubled k
    eo = pf["exponent in the other order"]
    assert any(v for k, v in eo.items() if k.startswith(("half=3 ", "half=160 ")))  # halves that are no power of two
    assert not any(v for k, v in eo.items() if k.startswith(("half=128 ", "half=512 ")))  # ... and only there: the orders coincide
    assert all(pf["cos and sin swapped"].values())
    tr = pf["truncating 2-byte store"]
    assert all(v for k, v in tr.items() if k.endswith(("tie_to_even_up", "tie_plus_ulp", "overflow_edge", "half_subnormal")))
    assert {k: v for k, v in pf["pad lanes unwritten"].items()} == {f"p={p} cs={cs}": cs > 3 * p * p for p in tc.PATCH_P for cs in tc.patch_strides(3, p)}
    ic = pf["index clamp missing"]
    assert ic["rows=6 idx=-5"] and ic["rows=6 idx=8"] and ic["rows=1 idx=3"] and not ic["rows=6 idx=0"] and not ic["rows=6 idx=5"]


# ------------------------------------------------------------------------------------------------ argument validation
def test_entries_validate_their_arguments():
    from azula_amd import _lib
    from azula_amd.csrc import build

    build.build()
    lib = _lib.lib()
    P, Q, Q8 = 0x1000, 0x1004, 0x1008  # 16-byte aligned / misaligned / 8-byte aligned addresses (never dereferenced: validation comes first)
    NULL, SHAPE, ALIGN = -1, -2, -3
    sw = lambda *a: lib.az_swiglu_f32(*a, None)  # noqa: E731
    #  y x rows cout xs ys
    assert sw(None, P, 4, 8, 16, 8) == NULL and sw(P, None, 4, 8, 16, 8) == NULL
    assert sw(P, P, 0, 8, 16, 8) == SHAPE and sw(P, P, 4, 0, 16, 8) == SHAPE
    assert sw(P, P, 4, 8, 14, 8) == SHAPE and sw(P, P, 4, 8, 16, 7) == SHAPE and sw(P, P, 4, 8, 17, 8) == SHAPE  # xs < 2 cout, ys < cout, odd xs
    assert sw(P, Q, 4, 8, 16, 8) == ALIGN and sw(P, Q, 4, 8, 18, 12) == ALIGN  # x not 8-byte aligned: the float2 loads
    pa = lambda *a: lib.az_patchify_f32(*a, None)  # noqa: E731
    un = lambda *a: lib.az_unpatchify_f32(*a, None)  # noqa: E731
    #  dst src scale B Z H W p cs   |   dst src B Z H W p cs
    assert pa(None, P, None, 1, 3, 8, 12, 2, 12) == NULL and pa(P, None, None, 1, 3, 8, 12, 2, 12) == NULL
    assert un(None, P, 1, 3, 8, 12, 2, 12) == NULL and un(P, None, 1, 3, 8, 12, 2, 12) == NULL
    for bad in ((0, 3, 8, 12, 2, 12), (1, 0, 8, 12, 2, 12), (1, 3, 8, 12, 0, 12), (1, 3, 9, 12, 2, 12), (1, 3, 8, 13, 2, 12), (1, 3, 8, 12, 2, 11)):
        assert pa(P, P, None, *bad) == SHAPE and un(P, P, *bad) == SHAPE, bad  # B, Z, p = 0; H % p; W % p; cs < Z p p
    tf = lambda *a: lib.az_token_fill_f32(*a, None)  # noqa: E731
    #  dst dst_tokens dst_off n row row_bstride pos B cs
    assert tf(None, 9, 0, 4, P, 24, P, 3, 24) == NULL and tf(P, 9, 0, 4, None, 24, P, 3, 24) == NULL and tf(P, 9, 0, 4, P, 24, None, 3, 24) == NULL
    for bad in ((9, 0, 4, P, 24, P, 0, 24), (9, 0, 0, P, 24, P, 3, 24), (9, 0, 4, P, 24, P, 3, 22), (9, 0, 4, P, 22, P, 3, 24),
                (9, -1, 4, P, 24, P, 3, 24), (9, 6, 4, P, 24, P, 3, 24)):  # B, n = 0; cs % 4; row_bstride % 4; window before / past the tokens
        assert tf(P, *bad) == SHAPE, bad
    assert tf(Q, 9, 0, 4, P, 24, P, 3, 24) == ALIGN and tf(P, 9, 0, 4, Q8, 24, P, 3, 24) == ALIGN and tf(P, 9, 0, 4, P, 24, Q, 3, 24) == ALIGN
    th = lambda *a: lib.az_token_fill_h16(*a, None)  # noqa: E731
    #  ... the same, then dtype
    assert th(None, 9, 0, 4, P, 24, P, 3, 24, 1) == NULL and th(P, 9, 0, 4, None, 24, P, 3, 24, 1) == NULL and th(P, 9, 0, 4, P, 24, None, 3, 24, 2) == NULL
    for bad in ((9, 0, 4, P, 24, P, 3, 20, 1), (9, 0, 4, P, 24, P, 3, 24, 0), (9, 0, 4, P, 24, P, 3, 24, 3), (9, 6, 4, P, 24, P, 3, 24, 2),
                (9, 0, 4, P, 22, P, 3, 24, 2), (9, 0, 4, P, 24, P, 0, 24, 2)):  # cs % 8; dtype 0, 3; window; row_bstride % 4; B = 0
        assert th(P, *bad) == SHAPE, bad
    assert th(Q8, 9, 0, 4, P, 24, P, 3, 24, 1) == ALIGN and th(P, 9, 0, 4, P, 24, Q, 3, 24, 2) == ALIGN
    te = lambda *a: lib.az_timestep_embedding_f32(*a, None)  # noqa: E731
    #  dst ldd t t_stride rows half max_period
    assert te(None, 256, P, 1, 5, 128, 1e4) == NULL and te(P, 256, None, 1, 5, 128, 1e4) == NULL
    for bad in ((255, P, 1, 5, 128, 1e4), (256, P, 2, 5, 128, 1e4), (256, P, -1, 5, 128, 1e4), (256, P, 1, 0, 128, 1e4), (256, P, 1, 5, 0, 1e4),
                (256, P, 1, 5, 128, 0.0), (256, P, 1, 5, 128, -2.0)):  # ldd < 2 half; t_stride; rows, half = 0; max_period <= 0
        assert te(P, *bad) == SHAPE, bad
    gr = lambda *a: lib.az_gather_rows_f32(*a, None)  # noqa: E731
    #  dst table idx nrows ncols table_rows
    assert gr(None, P, P, 4, 8, 6) == NULL and gr(P, None, P, 4, 8, 6) == NULL and gr(P, P, None, 4, 8, 6) == NULL
    assert gr(P, P, P, 0, 8, 6) == SHAPE and gr(P, P, P, 4, 0, 6) == SHAPE and gr(P, P, P, 4, 8, 0) == SHAPE
    gs = lambda *a: lib.az_gather_step_row_f32(*a, None)  # noqa: E731
    #  dst table coef which ncols table_rows
    assert gs(None, P, P, 0, 8, 6) == NULL and gs(P, None, P, 0, 8, 6) == NULL and gs(P, P, None, 1, 8, 6) == NULL
    assert gs(P, P, P, 0, 0, 6) == SHAPE and gs(P, P, P, 1, 8, 0) == SHAPE
    ls = lambda *a: lib.az_linear_small_f32(*a, None)  # noqa: E731
    #  y ldy x ldx W bias M N K in_act out_act
    assert ls(None, 7, P, 40, P, P, 5, 7, 40, 0, 0) == NULL and ls(P, 7, None, 40, P, P, 5, 7, 40, 0, 0) == NULL
    assert ls(P, 7, P, 40, None, None, 5, 7, 40, 0, 0) == NULL
    for bad in ((6, P, 40, P, None, 5, 7, 40, 0, 0), (7, P, 39, P, None, 5, 7, 40, 0, 0), (7, P, 40, P, None, 0, 7, 40, 0, 0),
                (7, P, 40, P, None, 5, 0, 40, 0, 0), (7, P, 40, P, None, 5, 7, 0, 0, 0)):  # ldy < N; ldx < K; M, N, K = 0
        assert ls(P, *bad) == SHAPE, bad
    lg = lambda *a: lib.az_linear_small_grouped_f32(*a, None)  # noqa: E731
    #  groups ngroups max_n M in_act out_act
    assert lg(None, 3, 256, 6, 0, 0) == NULL
    assert lg(P, 0, 256, 6, 0, 0) == SHAPE and lg(P, 65536, 256, 6, 0, 0) == SHAPE and lg(P, 3, 0, 6, 0, 0) == SHAPE and lg(P, 3, 256, 0, 0, 0) == SHAPE
    assert lib.az_silu_f32(None, P, 16, None) == NULL and lib.az_silu_f32(P, None, 16, None) == NULL and lib.az_silu_f32(P, P, 0, None) == SHAPE
    cf = lambda *a: lib.az_cfg_combine_f32(*a, None)  # noqa: E731
    #  y pos neg g n
    assert cf(None, P, P, P, 16) == NULL and cf(P, None, P, P, 16) == NULL and cf(P, P, None, P, 16) == NULL and cf(P, P, P, None, 16) == NULL
    assert cf(P, P, P, P, 0) == SHAPE


def test_grouped_linear_descriptors_are_checked_where_they_are_built():
    r"""``az_linear_small_grouped_f32`` reads its descriptors on the device and has the 16-byte kernel only: ``engine.linear_groups``
    (both callers: the modulation MLPs of engine.mod_front_tape, ADM's FiLM projections) raises before anything is launched."""
    from azula_amd import engine

    P = 0x1000
    ok = (P, P, P, None, 12, 64, 12, 64)  # y x W bias ldy ldx N K
    g = engine.linear_groups([ok, (P, P + 16 * 4, P, P, 16, 192, 12, 64)])
    assert len(g) == 2 and (g[0].K, g[0].N, g[0].ldx, g[0].bias) == (64, 12, 64, None) and (g[1].x, g[1].ldy, g[1].bias) == (P + 64, 16, P)
    for bad, why in (((P, P, P, None, 12, 62, 12, 62), "K % 4"), ((P, P, P, None, 12, 66, 12, 64), "ldx % 4"),
                     ((P, P + 4, P, None, 12, 64, 12, 64), "aligned x"), ((P, P, P + 8, None, 12, 64, 12, 64), "aligned x / W"),
                     ((P, P, P, None, 11, 64, 12, 64), "ldy"), ((P, P, P, None, 12, 60, 12, 64), "ldx"), ((P, 0, P, None, 12, 64, 12, 64), "null")):
        with pytest.raises(ValueError, match="group 1"):
            engine.linear_groups([ok, bad])
    with pytest.raises(ValueError, match="16-byte"):  # a modulation width that is no multiple of 4: the second block's x = h_all + 4 D bytes
        engine.linear_groups([(P, P + 4 * 30 * i, P, P, 12, 60, 12, 30) for i in range(2)])
