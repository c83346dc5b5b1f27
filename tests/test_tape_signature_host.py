r"""``tools/tape_signature.py::signature`` on hand-built tapes: equal for one structure at different base addresses, different
for a changed scalar, op order, offset into a buffer, or two temporaries swapping pool buffers -- so that "the signatures are
equal" says something.  No GPU: the tapes hold made-up addresses and are never run."""

import ctypes as C
import importlib.util
import os

from azula_amd._lib import AzConvArgs
from azula_amd.engine import Tape

_spec = importlib.util.spec_from_file_location(
    "tape_signature", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "tape_signature.py"))
ts = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ts)

SIZES = {"x": 4096, "pool0": 8192, "pool1": 8192, "w": 1024, "out": 4096}


def build(base: int, *, eps: float = 1e-5, offset: int = 256, swap: bool = False, reorder: bool = False):
    r"""(tape, allocations) of a plan whose buffers start at ``base``: a row norm x -> t0, a convolution t0 -> t1 (descriptor
    struct, weights read at ``offset`` bytes into ``w``), a layout pass t1 -> out; then, with both pool buffers free again,
    out -> t2 -> t3 -> x, where t2 and t3 take pool0 and pool1, or (``swap``) pool1 and pool0."""
    addr, p = {}, base
    for name, size in SIZES.items():
        addr[name] = p
        p += size + 512  # (gaps: an address between two buffers is in neither)
    t0, t1 = "pool0", "pool1"
    t2, t3 = ("pool1", "pool0") if swap else ("pool0", "pool1")
    a = AzConvArgs()
    a.src0, a.dst, a.weight = addr[t0], addr[t1], addr["w"] + offset
    a.batch, a.hin, a.win, a.ksize, a.c0s, a.cout_s = 2, 8, 8, 3, 16, 16
    a._flops, a._algo = 2 * 128 * 16 * 16 * 9, "az_conv2d_f32"
    ops = [
        (None, (addr[t0], addr["x"], None, 128, 16, eps), "az_rownorm_mod_f32"),
        (None, (C.byref(a),), "az_conv2d_f32"),
        (None, (addr["out"], addr[t1], 2, 16, 64, 16), "az_nhwc_to_nchw_f32"),
        (None, (addr[t2], addr["out"], None, 128, 16, eps), "az_rownorm_mod_f32"),
        (None, (addr[t3], addr[t2], 2048), "az_silu_f32"),
        (None, (addr["x"], addr[t3], 2, 16, 64, 16), "az_nhwc_to_nchw_f32"),
    ]
    if reorder:
        ops[0], ops[2] = ops[2], ops[0]
    tape = Tape()
    tape.ops.extend(ops)
    tape.keep.append(a)
    return tape, [(addr[n], SIZES[n]) for n in SIZES]


BASE_A, BASE_B = 0x7F0000000000, 0x7E8000400000


def sig(base=BASE_A, **kw):
    return ts.signature(*build(base, **kw))


def test_same_structure_at_other_addresses_is_equal():
    assert sig(BASE_A) == sig(BASE_B)
    s = sig()
    assert [op for op, _ in s][:3] == ["az_rownorm_mod_f32", "az_conv2d_f32", "az_nhwc_to_nchw_f32"]
    # allocations are numbered by first appearance (t0, x, then the descriptor's in field order), scalars and floats kept as they are
    assert s[0][1] == [["@", 0, 0], ["@", 1, 0], None, 128, 16, float(1e-5).hex()]
    conv = s[1][1][0]
    assert conv["struct"] == "AzConvArgs" and conv["src0"] == ["@", 0, 0] and conv["ksize"] == 3 and conv["bias"] is None
    assert sorted((conv["dst"], conv["weight"])) == [["@", 2, 0], ["@", 3, 256]] or sorted((conv["dst"], conv["weight"])) == [["@", 2, 256], ["@", 3, 0]]
    assert conv["_flops"] == 2 * 128 * 16 * 16 * 9 and conv["_algo"] == "az_conv2d_f32"
    assert s[2][1][:2] == [["@", 4, 0], conv["dst"]]


def test_changed_scalar_differs():
    assert sig(eps=1e-6) != sig()


def test_changed_op_order_differs():
    assert sig(reorder=True) != sig()


def test_other_offset_into_the_same_buffer_differs():
    assert sig(offset=512) != sig()


def test_temporaries_swapping_pool_buffers_differ():
    r"""The launches and every scalar are the same; the two later temporaries trade their (equally sized) pool buffers."""
    tape, allocs = build(BASE_A, swap=True)
    assert [op for op, _ in ts.signature(tape, allocs)] == [op for op, _ in sig()]
    assert ts.signature(tape, allocs) != sig()


def test_case_groups_selectable_with_only():
    assert list(ts.CASES) == ["unet", "adm", "dit", "jit", "samplers", "vdm", "unet3d", "vit.fused"] and all(callable(f) for f in ts.CASES.values())


def test_unknown_address_gets_an_ordinal_of_its_own():
    tape, allocs = build(BASE_A)
    known = ts.signature(tape, allocs)
    partial = ts.signature(tape, [a for a in allocs if a[0] != tape.ops[0][1][1]])  # without x
    assert partial[0][1][1] == ["?", 0, 0] and known[0][1][1] == ["@", 1, 0]
