r"""The two coefficient tables of the captured sampling loops are encodings of ONE walk over a sampling's denoiser evaluations
(``Sampler._fused_walk``): ``_host_table`` as AzStepCoef words (fp32), ``_host_table_wide`` as the 48-word fp64 row laid out by
``_lib.ROW64_*``.  Under an fp64 time grid every fp32 word must be the fp64 word rounded to fp32, bit for bit.  No GPU."""

import pytest
import torch

from azula_amd import _lib
from azula_amd import sample as S
from azula_amd.denoise import KarrasDenoiser
from azula_amd.noise import VPSchedule

DEN = KarrasDenoiser(torch.nn.Identity(), VPSchedule())
F64 = dict(dtype=torch.float64)
# name -> (sampler, denoiser evaluations per step)
SAMPLERS = {
    "ddpm": (lambda: S.DDPMSampler(DEN, steps=5, **F64), 1),
    "ddim": (lambda: S.DDIMSampler(DEN, steps=5, eta=0.5, **F64), 1),
    "euler": (lambda: S.EulerSampler(DEN, steps=5, **F64), 1),
    "heun": (lambda: S.HeunSampler(DEN, steps=4, **F64), 2),
    "ito": (lambda: S.ItoSampler(DEN, steps=5, eta=0.7, **F64), 1),
    "pc": (lambda: S.PCSampler(DEN, steps=3, corrections=2, **F64), 3),
    "zab": (lambda: S.zABSampler(DEN, order=3, steps=7, **F64), 1),
    "reab": (lambda: S.REABSampler(DEN, order=4, steps=7, **F64), 1),
    "vab": (lambda: S.vABSampler(DEN, order=2, steps=6, **F64), 1),
    "zeab": (lambda: S.zEABSampler(DEN, order=3, steps=6, **F64), 1),
    "xeab": (lambda: S.xEABSampler(DEN, order=3, steps=6, **F64), 1),
}
COL = {n: i for i, n in enumerate(_lib.COEF_FIELDS)}


def same_bits(a32: torch.Tensor, b64: torch.Tensor) -> bool:
    assert a32.dtype == torch.float32 and b64.dtype == torch.float64
    return torch.equal(a32.view(torch.int32), b64.to(torch.float32).view(torch.int32))


def test_row_layout():
    assert _lib.ROW64_FIELDS == _lib.COEF_FIELDS[:12] and len(_lib.ROW64_FIELDS) == 12
    assert (_lib.ROW64_DENOISER, _lib.ROW64_TRANSITION, _lib.ROW64_CLAMP, _lib.ROW64_SAMPLER, _lib.ROW64_WORDS) == (0, 12, 24, 36, 48)
    assert _lib.COEF_SPARE == (14, 15) and _lib.ROW64_SPARE == (4, 5) and S._FusedLoopWide.WORDS == 48
    assert _lib.row64_word("guidance", _lib.ROW64_CLAMP) == 35


@pytest.mark.parametrize("name", SAMPLERS)
def test_fp32_table_is_the_rounded_fp64_table(name):
    make, evaluations = SAMPLERS[name]
    smp = make()
    fused = S.FusedDenoiser(coefficients=DEN.host_coefficients, programs=[], guidance=1.5, clip=(-1.0, 1.0))
    t32, t64 = smp._host_table(fused), smp._host_table_wide(fused)
    rows = smp.steps * evaluations
    assert t32.shape == (rows, _lib.COEF_WORDS) and t64.shape == (rows, _lib.ROW64_WORDS)
    w = _lib.row64_word
    for block, fields in ((_lib.ROW64_DENOISER, ("c_in", "c_skip", "c_out", "c_time")),
                          (_lib.ROW64_TRANSITION, ("alpha_t", "alpha_s", "k_x", "k_eps")),
                          (_lib.ROW64_CLAMP, ("clip_lo", "clip_hi", "guidance"))):
        for f in fields:
            assert same_bits(t32[:, COL[f]], t64[:, w(f, block)]), (name, f)
    for spare32, spare64 in zip(_lib.COEF_SPARE, _lib.ROW64_SPARE):
        assert same_bits(t32[:, spare32], t64[:, spare64]), (name, spare32)
    # the clamp block: a transition row that only clips, with the CFG combination's constants in its unused slots
    for f, v in (("c_out", 1.0), ("alpha_s", 1.0), ("c_time", -1.0), ("c_in_next", 1.0)):
        assert torch.equal(t64[:, w(f, _lib.ROW64_CLAMP)], torch.full((rows,), v, dtype=torch.float64)), (name, f)
    # fp32 only: every evaluation pre-scales the next one's input, and every row carries its step number
    assert torch.equal(t32[:-1, COL["c_in_next"]], t32[1:, COL["c_in"]])
    assert t32.view(torch.int32)[:, COL["step"]].tolist() == [i for i in range(smp.steps) for _ in range(evaluations)]
    if hasattr(smp, "order"):
        ring, own, nh = smp._ring_table(), _lib.ROW64_SAMPLER, smp.order - 1
        assert own == 36 and ring.dtype == torch.float32
        assert same_bits(ring[:, :4], t64[:, own : own + 4]) and same_bits(ring[:, 4 : 4 + nh], t64[:, own + 4 : own + 4 + nh])
        assert torch.equal(t64[:, 47], torch.ones(rows, dtype=torch.float64))
