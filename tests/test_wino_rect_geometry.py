r"""Rectangular tile blocks of the x3 / f16x2 Winograd kernel (csrc/wino_x3.hip: RECT) -- the staging geometry on the host.

``az_winograd_x3_block_geometry`` runs the functions the kernel's prologue runs (csrc/conv_shared.h: ``X3RectGeom``) without a
device: for a block it returns the input pixel behind every staged slot and every tile's patch address.  Checked here against the
definition of the F(2x2, 3x3) gather: tile (th, tw) reads the 4 x 4 pixels (2 th - 1 + r, 2 tw - 1 + c)."""

import ctypes as C
import functools

import pytest

X_SLOTS = 768  # wino_x3.hip: pixel slots of the staging area
SLOTS_MAX = 512  # what the function fills (four staging pieces per thread)
RECTS = [(32, 2), (16, 4), (8, 8), (4, 16)]
MAPS = [(2, 2), (6, 6), (16, 16), (20, 12), (34, 18)]


@pytest.fixture(scope="module")
def lib():
    from azula_amd import _lib
    from azula_amd.csrc import build

    build.build()
    return _lib.lib()


def block_geometry(lib, batch, h, w, pad_mode, rw, rh, block):
    slot = (C.c_int32 * (3 * SLOTS_MAX))()
    tile = (C.c_int32 * (4 * 64))()
    n = lib.az_winograd_x3_block_geometry(batch, h, w, pad_mode, rw, rh, block, C.addressof(slot), C.addressof(tile))
    assert n > 0, n
    slots = [tuple(slot[3 * s : 3 * s + 3]) for s in range(SLOTS_MAX)]
    tiles = [tuple(tile[4 * j : 4 * j + 4]) for j in range(64)]
    return n, slots, tiles


def choose(lib, batch, h, w, whole=0):
    rw, rh = C.c_int32(), C.c_int32()
    slots, run = C.c_int64(), C.c_int64()
    rc = lib.az_winograd_x3_choose_block(batch, h, w, whole, C.addressof(rw), C.addressof(rh), C.addressof(slots), C.addressof(run))
    assert rc == 0, rc
    return rw.value, rh.value, slots.value, run.value


def expected_pixel(b, i, j, h, w, pad_mode):
    r"""What a staged slot for input coordinates (i, j) of image b must hold: the wrapped pixel under circular padding, zeros
    (-1, -1, -1) out of bounds."""
    if pad_mode:
        return (b, i % h, j % w)
    return (b, i, j) if 0 <= i < h and 0 <= j < w else (-1, -1, -1)


@pytest.mark.parametrize("pad_mode", [0, 1])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("h,w", MAPS)
@pytest.mark.parametrize("rw,rh", RECTS)
def test_every_tile_reads_its_patch_from_the_staged_window(lib, rw, rh, h, w, batch, pad_mode):
    tiles_h, tiles_w = (h + 1) // 2, (w + 1) // 2
    bpi = -(-tiles_h // rh) * -(-tiles_w // rw)
    ws = 2 * rw + 2
    seen = {}
    for block in range(batch * bpi):
        n, slots, tiles = block_geometry(lib, batch, h, w, pad_mode, rw, rh, block)
        assert n == (2 * rh + 2) * ws and n <= SLOTS_MAX < X_SLOTS
        assert all(s == (-1, -1, -1) for s in slots[n:]), "slots behind the window stage zeros"
        images = {s[0] for s in slots if s[0] >= 0} | {t[0] for t in tiles if t[0] >= 0}
        assert images <= {block // bpi}, (block, images)  # one image per block
        for j, (b, th, tw, ps) in enumerate(tiles):
            assert ps == 2 * (j // rw) * ws + 2 * (j % rw)  # a wave's eight tiles are neighbours along the row (rw >= 8)
            assert 0 <= ps and ps + 3 * ws + 3 < n  # the patch of a masked tile stays inside the window too
            if b < 0:
                assert th >= tiles_h or tw >= tiles_w, (block, j, th, tw)
                continue
            assert b == block // bpi and 0 <= th < tiles_h and 0 <= tw < tiles_w
            assert (b, th, tw) not in seen, ("tile in two blocks", b, th, tw, seen.get((b, th, tw)), block)
            seen[(b, th, tw)] = block
            for r in range(4):
                for c in range(4):
                    got = slots[ps + r * ws + c]
                    assert got == expected_pixel(b, 2 * th - 1 + r, 2 * tw - 1 + c, h, w, pad_mode), (block, j, r, c, got)
    assert len(seen) == batch * tiles_h * tiles_w, "every tile exactly once"


def test_run_form_has_no_rectangle_geometry(lib):
    slot = (C.c_int32 * (3 * SLOTS_MAX))()
    tile = (C.c_int32 * (4 * 64))()
    args = (C.addressof(slot), C.addressof(tile))
    assert lib.az_winograd_x3_block_geometry(1, 16, 16, 0, 64, 1, 0, *args) == -4  # AZ_E_UNSUPPORTED: the run form is not a rectangle
    assert lib.az_winograd_x3_block_geometry(1, 16, 16, 0, 8, 4, 0, *args) == -4  # not one of the shapes
    assert lib.az_winograd_x3_block_geometry(1, 16, 16, 0, 8, 8, 1, *args) == -2  # one block only
    assert lib.az_winograd_x3_block_geometry(1, 16, 16, 0, 8, 8, 0, None, None) == -1


@functools.lru_cache(None)
def run_form_slots(batch, tiles_h, tiles_w):
    r"""Staged slots of the run form, block by block: a block's 64 consecutive tiles (tile rows follow each other across images)
    fall into runs of one tile row each; a run of n tiles stages 4 (2 n + 2) slots."""
    ntiles, total = batch * tiles_h * tiles_w, 0
    for t0 in range(0, ntiles, 64):
        rows = {}
        for t in range(t0, t0 + 64):  # (the tiles past the end of the last block are staged like any other)
            rows[t // tiles_w] = rows.get(t // tiles_w, 0) + 1
        total += sum(4 * (2 * n + 2) for n in rows.values())
    return total


@pytest.mark.parametrize("whole", [0, 1])
@pytest.mark.parametrize("batch", [1, 3, 4])
@pytest.mark.parametrize("h,w", MAPS + [(32, 32), (64, 64), (256, 256), (40, 40), (32, 16)])
def test_the_chooser_never_stages_more_than_the_run_form(lib, h, w, batch, whole):
    tiles_h, tiles_w = (h + 1) // 2, (w + 1) // 2
    rw, rh, slots, run = choose(lib, batch, h, w, whole)
    assert run == run_form_slots(batch, tiles_h, tiles_w)
    assert (rw, rh) in RECTS + [(64, 1)] and slots <= run
    run_blocks = -(-batch * tiles_h * tiles_w // 64)
    if rh == 1:
        assert slots == run
    else:
        blocks = batch * -(-tiles_h // rh) * -(-tiles_w // rw)
        assert slots == blocks * (2 * rw + 2) * (2 * rh + 2) and slots < run  # (a tie goes to the run form)
        assert blocks <= run_blocks  # never more workgroups: each streams its whole filter chunk
        if whole:
            assert tiles_h % rh == 0 and tiles_w % rw == 0
    # the choice is the minimum over the admissible shapes
    for cw, ch in RECTS:
        blocks = batch * -(-tiles_h // ch) * -(-tiles_w // cw)
        if blocks <= run_blocks and not (whole and (tiles_h % ch or tiles_w % cw)):
            assert slots <= blocks * (2 * cw + 2) * (2 * ch + 2), (cw, ch)


def test_the_flagship_shapes_take_the_square(lib):
    r"""The maps of the 256 x 256 UNet at batch 4 (128^2 ... 8^2 tiles, then 4^2): 8 x 8 tiles = 324 slots per block wherever an image holds
    whole squares; below that (16 tiles per image) the run form stays."""
    for hw, run_per_block in ((256, 520), (128, 520), (64, 528), (32, 544), (16, 576)):
        rw, rh, slots, run = choose(lib, 4, hw, hw, 1)
        blocks = 4 * (hw // 2) ** 2 // 64
        assert (rw, rh) == (8, 8) and slots == 324 * blocks and run == run_per_block * blocks, (hw, rw, rh, slots, run)
    assert choose(lib, 4, 8, 8)[:2] == (64, 1)
