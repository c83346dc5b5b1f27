r"""RePaintSampler on the GPU: ``az_repaint_f32`` against the torch op sequence bit for bit, the captured loop against the
restatement of ``tests/repaint_oracle.py`` fed the noise the device drew (same seed, same order), the generator state after
sampling, fused against the generic loop, ADM / CFG denoisers, per-call re-reads of ``y`` / ``mask``, and the fp64 clock."""

import ctypes

import pytest
import torch

import repaint_oracle
from conftest import max_err
from oracle import nets, sampling, synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------------------- kernel
def _coef():
    return [torch.tensor(v, dtype=torch.float32) for v in (0.7310586, 0.6819212, 1.3702, 0.4123)]


def _launch(x_s, y, mask, n_y, n_x, coef, xs_out=None, xt_out=None):
    from azula_amd import _lib

    a = _lib.AzRepaintArgs(x_s=x_s.data_ptr(), y=y.data_ptr(), mask=mask.data_ptr(), n_y=n_y.data_ptr(),
                           n_x=n_x.data_ptr() if n_x is not None else None, x_s_out=xs_out.data_ptr() if xs_out is not None else None,
                           x_t_out=xt_out.data_ptr() if xt_out is not None else None, coef=coef.data_ptr(), n=x_s.numel())
    _lib.call("az_repaint_f32", ctypes.byref(a), _lib.stream_ptr())


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a[~nan], b[~nan])


@pytest.mark.parametrize("n", [4 * 5000, 4 * 5000 + 3, 7, 4 * 1024 * 256 * 3 + 4 * 17])
def test_kernel_is_the_torch_op_sequence(n):
    g = torch.Generator().manual_seed(n)
    x, y, ny, nx = (torch.randn(n, generator=g) * 3 for _ in range(4))
    m = torch.rand(n, generator=g) < 0.5
    m[5], m[6] = True, False
    x[5] = float("nan")  # under the mask: selected away (a select, not a blend)
    x[6] = float("nan")  # outside it: kept, as torch.where keeps it
    a_s, s_s, ratio, kick = _coef()
    ref_s = torch.where(m, a_s * y + s_s * ny, x)
    ref_t = ratio * ref_s + kick * nx
    assert not torch.isnan(ref_s[5]) and torch.isnan(ref_s[6])
    coef = torch.stack(_coef()).cuda()
    d = {k: v.cuda() for k, v in dict(x=x, y=y, m=m, ny=ny, nx=nx).items()}
    xs_out, xt_out = torch.full_like(d["x"], 7.0), torch.full_like(d["x"], 7.0)
    _launch(d["x"], d["y"], d["m"], d["ny"], d["nx"], coef, xs_out, xt_out)
    assert _same_bits(xs_out, ref_s) and _same_bits(xt_out, ref_t)
    # the last iteration: x_t_out = NULL, n_x not read (a NULL n_x), x_s' in place
    xs = d["x"].clone()
    _launch(xs, d["y"], d["m"], d["ny"], None, coef, xs_out=xs)
    assert _same_bits(xs, ref_s)
    # a non-last iteration in place: x_t' over x_s
    xt = d["x"].clone()
    _launch(xt, d["y"], d["m"], d["ny"], d["nx"], coef, xt_out=xt)
    assert _same_bits(xt, ref_t)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- helpers
def _unet(g):
    from test_gpu_fp64 import unet_denoiser

    cfg = g.meta["unet_cfg"]
    sd = synth.synth_state_dict({k: tuple(v) for k, v in g.meta["unet_shapes"].items()}, g.meta["unet_weight_seed"])
    omean = lambda x, t: sampling.karras_mean(lambda a, c: nets.time_wrapped_unet(sd, cfg, a, c), x, t)  # noqa: E731
    return unet_denoiser(g), omean


def _device_noise(seed, steps, iterations, x_shape, y_shape, dtype=torch.float32, first=torch.float32):
    r"""The generator calls of the reference, made on the device: per iteration randn_like(x_t), randn_like(y),
    randn_like(x_s); (fp64 clock: x_t / x_s are fp64 except the very first x_t of an fp32 input)."""
    torch.manual_seed(seed)
    out = []
    for i in range(steps * iterations):
        out += [torch.randn(x_shape, device="cuda", dtype=first if i == 0 else dtype), torch.randn(y_shape, device="cuda"),
                torch.randn(x_shape, device="cuda", dtype=dtype)]
    return [e.cpu() for e in out], torch.cuda.get_rng_state()


def _loop(smp):
    assert len(smp._fused_cache) == 1
    return next(iter(smp._fused_cache.values()))


def _unet_case(golden):
    g = golden("g25_repaint")
    den, omean = _unet(g)
    return g, den, omean, g["unet_it3_x1"], g["unet_it3_y"], g["unet_it3_mask"]


# ------------------------------------------------------------------------------------------------------------- captured loop
def test_unet_captured_loop_matches_the_restatement(golden):
    from azula_amd.guidance import RePaintSampler
    from azula_amd.sample import _FusedLoop

    g, den, omean, x1, y, mask = _unet_case(golden)
    smp = RePaintSampler(den, y.cuda(), mask.cuda(), steps=8, iterations=3, silent=True)
    torch.manual_seed(11)
    x0 = smp(x1.cuda())
    state = torch.cuda.get_rng_state()
    loop = _loop(smp)
    assert type(loop) is _FusedLoop and loop.n_rows == 24 and loop.graph is not None
    names = [op[2] for op in loop.tape.ops]
    assert names.count("az_repaint_f32") == 3 and names.count("az_step_begin") == 3 and names.count("az_gather_step_row_f32") == 1
    noise, ref_state = _device_noise(11, 8, 3, x1.shape, y.shape)
    ref = repaint_oracle.sample_repaint(omean, x1, y, mask, steps=8, iterations=3, eta=0.0, noise=noise)
    err, sc = max_err(x0, ref), max(1.0, ref.abs().max().item())
    print("RePaint UNet DDIM-8 x 3, captured loop vs restatement: max|d|", err, "scale", sc)
    assert err < 5e-4 * sc
    assert torch.equal(state, ref_state)  # 3 x iterations draws per step, the last re-noise and the eta = 0 draws included
    torch.manual_seed(11)
    assert torch.equal(smp(x1.cuda()), x0) and _loop(smp) is loop


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_fused_equals_the_generic_loop(golden, eta):
    from azula_amd.guidance import RePaintSampler

    class Generic(RePaintSampler):
        def step(self, x_t, t, s, **kw):
            return super().step(x_t, t, s, **kw)

    g, den, omean, x1, y, mask = _unet_case(golden)  # (mask: (1, 1, H, W), broadcast)
    out, states = [], []
    for cls in (RePaintSampler, Generic):
        smp = cls(den, y.cuda(), mask.cuda(), steps=8, iterations=3, eta=eta, silent=True)
        torch.manual_seed(5)
        out.append(smp(x1.cuda()))
        states.append(torch.cuda.get_rng_state())
        assert bool(smp._fused_cache) == (cls is RePaintSampler)
    err, sc = max_err(out[0], out[1]), max(1.0, out[1].abs().max().item())
    print(f"eta {eta}: fused vs generic max|d|", err, "scale", sc)
    assert err < 1e-4 * sc and torch.equal(states[0], states[1])


def test_generic_loop_with_a_broadcast_observation(golden):
    r"""``y`` of shape (1, C, H, W): the generic loop, whose observation noise is drawn in y's shape and then expanded."""
    from azula_amd.guidance import RePaintSampler

    g, den, omean, x1, y, mask = _unet_case(golden)
    y1 = y[:1].contiguous()
    smp = RePaintSampler(den, y1.cuda(), mask.cuda(), steps=4, iterations=2, eta=0.3, silent=True)
    torch.manual_seed(6)
    x0 = smp(x1.cuda())
    state = torch.cuda.get_rng_state()
    assert not smp._fused_cache
    noise, ref_state = _device_noise(6, 4, 2, x1.shape, y1.shape)
    ref = repaint_oracle.sample_repaint(omean, x1, y1, mask, steps=4, iterations=2, eta=0.3, noise=noise)
    err, sc = max_err(x0, ref), max(1.0, ref.abs().max().item())
    print("generic, broadcast y: max|d|", err, "scale", sc)
    assert err < 5e-4 * sc and torch.equal(state, ref_state)


def test_y_and_mask_are_read_on_every_call(golden):
    from azula_amd.guidance import RePaintSampler

    g, den, omean, x1, y, mask = _unet_case(golden)
    yd, md = y.cuda(), mask.cuda()
    smp = RePaintSampler(den, yd, md, steps=4, iterations=2, silent=True)
    torch.manual_seed(3)
    first = smp(x1.cuda())
    loop = _loop(smp)
    yd.mul_(-0.5)  # in place: the same tensors, new values
    md[..., 0:3, :] = True
    torch.manual_seed(3)
    x0 = smp(x1.cuda())
    assert _loop(smp) is loop and not torch.equal(x0, first)
    noise, _ = _device_noise(3, 4, 2, x1.shape, y.shape)
    ref = repaint_oracle.sample_repaint(omean, x1, yd.cpu(), md.cpu(), steps=4, iterations=2, noise=noise)
    err, sc = max_err(x0, ref), max(1.0, ref.abs().max().item())
    print("after in-place edits: max|d|", err)
    assert err < 5e-4 * sc
    # a new y shape (and batch): a new plan
    smp.y, smp.mask = yd[:1].contiguous(), md
    torch.manual_seed(3)
    x0 = smp(x1[:1].cuda())
    assert _loop(smp) is not loop
    noise, _ = _device_noise(3, 4, 2, x1[:1].shape, (1, *y.shape[1:]))
    ref = repaint_oracle.sample_repaint(omean, x1[:1], yd[:1].cpu(), md.cpu(), steps=4, iterations=2, noise=noise)
    assert max_err(x0, ref) < 5e-4 * max(1.0, ref.abs().max().item())


def test_adm_learned_variance_on_the_captured_loop(golden):
    from test_gpu_adm import _adm_oracle, build

    from azula_amd.guidance import RePaintSampler

    g = golden("g5_adm_uncond")
    den, sd, cfg = build(g)
    omean, sched = _adm_oracle(g, sd, cfg)
    x1 = g["x1"]
    gen = torch.Generator().manual_seed(8)
    mask = torch.zeros(1, 1, *x1.shape[2:], dtype=torch.bool)
    mask[..., 8:24, 4:20] = True
    y = (torch.rand(x1.shape, generator=gen) * 1.6 - 0.8) * mask
    smp = RePaintSampler(den, y.cuda(), mask.cuda(), steps=4, iterations=2, silent=True)
    torch.manual_seed(4)
    x0 = smp(x1.cuda())
    state = torch.cuda.get_rng_state()
    loop = _loop(smp)
    assert loop.graph is not None and loop.fused.programs[0].f_channels == 2 * x1.shape[1]
    noise, ref_state = _device_noise(4, 4, 2, x1.shape, y.shape)
    ref = repaint_oracle.sample_repaint(omean, x1, y, mask, schedule=sched, steps=4, iterations=2, noise=noise)
    err, sc = max_err(x0, ref), max(1.0, ref.abs().max().item())
    print("ADM RePaint DDIM-4 x 2 vs restatement: max|d|", err, "scale", sc)
    assert err < 5e-4 * sc and torch.equal(state, ref_state)


def test_cfg_fused_equals_generic(golden):
    from test_gpu_adm import build

    from azula_amd.guidance import CFGDenoiser, RePaintSampler

    class Generic(RePaintSampler):
        def step(self, x_t, t, s, **kw):
            return super().step(x_t, t, s, **kw)

    g = golden("g5_adm_cond_neworder")
    den, _, _ = build(g)
    cfgden = CFGDenoiser(den)
    x1 = g["x1"].cuda()
    mask = torch.zeros(1, 1, *x1.shape[2:], dtype=torch.bool, device="cuda")
    mask[..., :, : x1.shape[-1] // 2] = True
    y = 0.5 * torch.ones_like(x1) * mask
    kwargs = dict(positive={"label": g["y"].cuda()}, negative={"label": g["neg_label"].cuda()}, guidance=2.0)
    out = []
    for cls in (RePaintSampler, Generic):
        smp = cls(cfgden, y, mask, steps=4, iterations=2, silent=True)
        torch.manual_seed(7)
        out.append(smp(x1, **kwargs))
        if cls is RePaintSampler:
            loop = _loop(smp)
            assert loop.graph is not None and len(loop.fused.programs) == 2
    err = max_err(out[0], out[1])
    print("CFG RePaint fused vs generic: max|d|", err)
    assert err < 6e-4  # (the bound of test_cfg_ddim16_fused_and_generic: c_out = -100 at t = 1 amplifies scalar ulps)


def test_fp64_clock_on_the_device(golden):
    from azula_amd.guidance import RePaintSampler

    g, den, omean, x1, y, mask = _unet_case(golden)
    smp = RePaintSampler(den, y.cuda(), mask.cuda(), steps=4, iterations=2, eta=0.2, silent=True, dtype=torch.float64)
    torch.manual_seed(12)
    x0 = smp(x1.cuda())
    state = torch.cuda.get_rng_state()
    assert x0.dtype == torch.float64 and not smp._fused_cache
    noise, ref_state = _device_noise(12, 4, 2, x1.shape, y.shape, dtype=torch.float64)
    ref = repaint_oracle.sample_repaint(omean, x1, y, mask, steps=4, iterations=2, eta=0.2, dtype=torch.float64, noise=noise)
    assert ref.dtype == torch.float64
    err, sc = max_err(x0, ref), max(1.0, ref.abs().max().item())
    print("fp64 clock vs restatement: max|d|", err, "scale", sc)
    assert err < 1e-4 * sc and torch.equal(state, ref_state)
    # the fp32 sampler on the same observation: the same trajectory up to fp32 round-off and its different noise draws
    torch.manual_seed(12)
    x32 = RePaintSampler(den, y.cuda(), mask.cuda(), steps=4, iterations=2, eta=0.2, silent=True)(x1.cuda())
    assert x32.dtype == torch.float32
    m = mask.expand(x1.shape).cuda()
    print("fp64 vs fp32 on observed pixels: max|d|", max_err(x0[m], x32[m]))
    assert torch.isfinite(x0).all() and torch.isfinite(x32).all()
