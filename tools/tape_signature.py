r"""Address-free signatures of kernel tapes: "same launches, same arguments, same buffer aliasing" as a comparison.

``signature(tape, allocations)`` turns every op of a :class:`azula_amd.engine.Tape` into plain data: the entry name, every
scalar argument as it is (floats by ``float.hex``), every ctypes struct argument field by field (plus its ``_flops`` /
``_algo`` attributes).  Every device or host address becomes ``["@", ordinal, byte offset]``: the ordinal of the allocation
it falls in, allocations numbered by their first appearance on the tape, so two builds of one plan at different base
addresses give equal signatures, and a tensor that lands in another buffer, or at another offset, does not.  An address in
no known allocation gets an ordinal of its own (``["?", n, 0]``) by first appearance.  Positional integers of at least 2^32
are addresses; no size on the plans of this package reaches that.  What a kernel reads through a table on the device (the
descriptors of ``az_linear_small_grouped_f32``) is not on the tape; the bit-equal outputs cover it.

    python tools/tape_signature.py run DIR [--only unet,adm,dit,jit,samplers,vdm,unet3d,vit.fused]    # builds the plans below, writes signatures + outputs
    python tools/tape_signature.py compare DIR_A DIR_B                  # equal signatures?  bit-equal outputs?
"""

from __future__ import annotations

import bisect
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDRESS_MIN = 1 << 32


# ------------------------------------------------------------------------------------------------ the pure part
def _ranges(allocations) -> list[tuple[int, int]]:
    r"""(start, end) byte ranges, sorted: of ``(address, bytes)`` pairs or of tensors (their whole storage)."""
    out = set()
    for a in allocations:
        if isinstance(a, tuple):
            start, size = a
        else:
            st = a.untyped_storage()
            start, size = st.data_ptr(), st.nbytes()
        if start and size:
            out.add((int(start), int(start) + int(size)))
    return sorted(out)


class _Resolver:
    def __init__(self, allocations) -> None:
        self.ranges = _ranges(allocations)
        self.starts = [r[0] for r in self.ranges]
        self.ordinal: dict[int, int] = {}  # range start -> ordinal
        self.unknown: dict[int, int] = {}  # address -> ordinal

    def address(self, p: int) -> list:
        i = bisect.bisect_right(self.starts, p) - 1
        if i >= 0 and p < self.ranges[i][1]:
            start = self.ranges[i][0]
            return ["@", self.ordinal.setdefault(start, len(self.ordinal)), p - start]
        return ["?", self.unknown.setdefault(p, len(self.unknown)), 0]

    def value(self, v, pointer: bool = False):
        if v is None:
            return None
        if isinstance(v, bool):
            return int(v)
        if isinstance(v, float):
            return float(v).hex()
        if isinstance(v, int):
            return self.address(v) if (v >= ADDRESS_MIN or (pointer and v)) else v
        if isinstance(v, (bytes, str)):
            return repr(v)
        if isinstance(v, C.Array):
            return [self.value(e) for e in v]
        if isinstance(v, C.Structure):
            return self.struct(v)
        if hasattr(v, "_obj"):  # ctypes.byref(struct)
            return self.struct(v._obj)
        raise TypeError(f"tape argument of type {type(v).__name__}")

    def struct(self, s) -> dict:
        d = {"struct": type(s).__name__}
        for name, ctype, *_ in s._fields_:
            d[name] = self.value(getattr(s, name), pointer=ctype is C.c_void_p)
        for extra in ("_flops", "_algo"):  # (plain values: an operation count may pass 2^32 and is no address)
            if hasattr(s, extra):
                d[extra] = getattr(s, extra)
        return d

    def ops(self, tape) -> list:
        return [[name, [self.value(a) for a in args]] for _, args, name in tape.ops]


def signature(tape, allocations) -> list:
    r"""Per op ``[entry name, [argument, ...]]`` with every address rewritten as described above.  Pure: reads ``tape.ops``
    and the allocations' address ranges, calls nothing."""
    return _Resolver(allocations).ops(tape)


def mask_ordinals(sig, ordinals: set):
    r"""``sig`` with the given allocation ordinals blanked (which pool buffer a temporary landed in), offsets kept."""
    if isinstance(sig, list):
        if len(sig) == 3 and sig[0] == "@" and sig[1] in ordinals:
            return ["@", "pool", sig[2]]
        return [mask_ordinals(v, ordinals) for v in sig]
    if isinstance(sig, dict):
        return {k: mask_ordinals(v, ordinals) for k, v in sig.items()}
    return sig


# ------------------------------------------------------------------------------------------------ plans -> allocations
def tensors_of(*roots) -> list:
    r"""Every tensor reachable from the plans' own objects: pools, ``tape.keep`` lists, packed weights, static buffers."""
    import torch

    found, seen, todo = [], set(), list(roots)
    while todo:
        o = todo.pop()
        if o is None or id(o) in seen or isinstance(o, (int, float, str, bytes, bool, C.Structure, C.Array)):
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            found.append(o)
        elif isinstance(o, torch.nn.Module):
            found.extend(o.parameters())
            found.extend(o.buffers())
        elif isinstance(o, (list, tuple, set)):
            todo.extend(o)
        elif isinstance(o, dict):
            todo.extend(o.values())
        elif type(o).__module__.startswith("azula_amd"):
            todo.extend(getattr(o, "__dict__", {}).values())
            todo.extend(getattr(o, s, None) for s in getattr(type(o), "__slots__", ()))
    return found


def _allocator_blocks() -> list:
    r"""``(address, bytes)`` of every block of torch's caching allocator: each tensor allocation is one block, at its address."""
    import torch

    out = []
    for seg in torch.cuda.memory_snapshot():
        at = seg["address"]
        for blk in seg["blocks"]:
            out.append((at, blk["size"]))
            at += blk["size"]
    return out


def plan_record(plan, module=None) -> dict:
    r"""Signatures of one plan: a forward plan (``.tape``, or a standalone block's tuple), or a gradient plan (``.fwd``, ``.bwd``)."""
    tapes = {}
    allocs = tensors_of(plan, module, getattr(plan, "roots", None))
    if isinstance(plan, tuple):  # UNetBlock's one-block plans on older checkouts: (x_in, mod, tape, out)
        tapes["tape"] = plan[2]
        allocs = allocs + _allocator_blocks()  # (a tuple does not expose its pool: the temporaries are the allocator's own blocks)
    elif hasattr(plan, "fwd"):
        tapes["fwd"], tapes["bwd"] = plan.fwd, plan.bwd
    else:
        tapes["tape"] = plan.tape
    pool = getattr(getattr(plan, "bld", None), "pool", None)
    pool_starts = {t.untyped_storage().data_ptr() for t in pool.all} if pool is not None else set()
    rec = {}
    for name, tape in tapes.items():
        r = _Resolver(allocs)
        rec[name] = r.ops(tape)
        rec[name + "_pool_ordinals"] = sorted(n for start, n in r.ordinal.items() if start in pool_starts)
    if hasattr(plan, "saved_bytes"):
        rec["saved_bytes"] = plan.saved_bytes
    return rec


# ------------------------------------------------------------------------------------------------ the cases
def _golden(name):
    import numpy as np
    import torch

    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}


def _synth(meta):
    from oracle import synth

    return synth.synth_state_dict({k: tuple(v) for k, v in meta["shapes"].items()}, meta["weight_seed"])


def _randomise(module, seed: int) -> None:
    r"""Zero-initialised layers (ADM's output convolutions, adaLN projections) get values: a zero weight hides its input."""
    import math

    import torch

    g = torch.Generator().manual_seed(seed)
    for _, v in sorted(module.state_dict().items()):
        if torch.is_floating_point(v) and v.ndim > 1 and not torch.any(v != 0):
            v.copy_(torch.randn(v.shape, generator=g) / math.sqrt(v[0].numel()))


class Recorder:
    def __init__(self, out_dir: str) -> None:
        self.dir = out_dir
        os.makedirs(out_dir, exist_ok=True)
        self.index: list[str] = []

    def save(self, case: str, module, outputs: dict, plans=None) -> None:
        r"""Signatures of every plan ``module`` holds (or of ``plans``), and the outputs as .npy."""
        import numpy as np

        rec = {}
        for plan in (plans if plans is not None else module._plans).values():  # (insertion order: the order of the calls)
            kind = "grad" if hasattr(plan, "fwd") else "forward"
            n = sum(k.startswith(kind) for k in rec)
            rec[f"{kind}{n}"] = plan_record(plan, module)
        with open(os.path.join(self.dir, case + ".json"), "w") as f:
            json.dump(rec, f)
        for k, t in outputs.items():
            np.save(os.path.join(self.dir, f"{case}.{k}.npy"), t.detach().float().cpu().numpy())
        self.index.append(case)
        sizes = [k + " " + "+".join(str(len(v[t])) for t in ("tape", "fwd", "bwd") if t in v) + " ops" for k, v in rec.items()]
        print(case + ": " + ", ".join(sizes), flush=True)


class _LoopTape:
    r"""One step of a captured sampling loop as a forward plan: its tape, and where its allocations are found."""

    def __init__(self, tape, roots) -> None:
        self.tape, self.roots = tape, roots


def _cotangent(out, seed: int = 7):
    import torch

    return torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _fwd_vjp(rec: Recorder, case: str, net, *args) -> None:
    y = net(*args)
    out, pull = net.vjp(*args)
    rec.save(case, net, {"y": y, "vjp_out": out, "dx": pull(_cotangent(out))})


def unet_cases(rec: Recorder) -> None:
    import torch

    from azula_amd.nn import UNet, UNetBlock

    for name in ("unet_group", "unet_layer_odd", "unet_rms_nomod"):
        meta, g = _golden("g5_" + name)
        cfg = meta["cfg"]
        net = UNet(cfg["in_channels"], cfg["out_channels"], hid_channels=cfg["hid_channels"], hid_blocks=cfg["hid_blocks"],
                   norm=cfg["norm"], groups=cfg["groups"], mod_features=cfg["mod_features"])
        net.load_state_dict(_synth(meta))
        net = net.cuda().eval()
        mod = g["modB"].cuda() if "modB" in g else None
        _fwd_vjp(rec, "unet." + name, net, g["x"].cuda(), mod)
    gen = torch.Generator().manual_seed(11)
    kw = dict(hid_channels=(8, 16), hid_blocks=(1, 1), norm="group", groups=4, mod_features=16)
    variants = {
        "stride3": (dict(stride=3), (2, 3, 18, 18)), "spatial1": (dict(spatial=1), (2, 3, 32)),
        "periodic": (dict(periodic=True), (2, 3, 16, 16)), "bf16": (dict(), (2, 3, 16, 16)),
    }
    for name, (extra, shape) in variants.items():
        torch.manual_seed(12)
        net = UNet(3, 3, **kw, **extra).cuda().eval()
        x, mod = torch.randn(shape, generator=gen).cuda(), torch.randn(2, 16, generator=gen).cuda()
        if name == "bf16":  # (groups of 4 and 8 channels: the activations stay in the module's type)
            net = UNet(3, 3, **{**kw, "groups": 2}).cuda().eval().bfloat16()
            x, mod = x.bfloat16(), mod.bfloat16()
        rec.save("unet." + name, net, {"y": net(x, mod)})
    torch.manual_seed(13)
    blk = UNetBlock(16, mod_features=16, norm="group", groups=4).cuda().eval()
    x, mod = torch.randn(2, 16, 12, 12, generator=gen).cuda(), torch.randn(2, 16, generator=gen).cuda()
    _fwd_vjp(rec, "unet.block", blk, x, mod)
    torch.manual_seed(14)
    blk3 = UNetBlock(16, mod_features=16, norm="group", groups=4, spatial=3, kernel_size=(3, 3, 3)).cuda().eval()
    rec.save("unet.block3d", blk3, {"y": blk3(torch.randn(2, 16, 4, 8, 8, generator=gen).cuda(), mod)})


def _adm(meta):
    from azula_amd.plugins import adm

    den = adm.make_model(**meta["cfg"])
    den.backbone.load_state_dict(_synth(meta))
    return den.cuda().eval()


def adm_cases(rec: Recorder) -> None:
    import torch

    from azula_amd.plugins import adm
    from azula_amd.sample import DDIMSampler

    for name in ("g5_adm_uncond", "g14_adm_plain_conv", "g24_adm_hd24_legacy"):
        meta, g = _golden(name)
        net = _adm(meta).backbone
        _fwd_vjp(rec, "adm." + name, net, g["x"].cuda(), g["idx"].cuda(), g["y"].cuda() if "y" in g else None)
    gen = torch.Generator().manual_seed(21)
    small = dict(image_size=16, num_channels=32, channel_mult=(1, 2), attention_resolutions=(8,), num_res_blocks=2,
                 num_head_channels=32, resblock_updown=True, use_scale_shift_norm=True)

    def make(seed=0, **kw):
        torch.manual_seed(seed)
        den = adm.make_model(**{**small, **kw})
        _randomise(den.backbone, 123)
        return den.cuda().eval().backbone

    net = make(num_classes=10)
    x = torch.randn(2, 3, 16, 16, generator=gen).cuda()
    rec.save("adm.cond_per_sample_t", net, {"y": net(x, torch.tensor([5, 700]).cuda(), torch.tensor([1, 7]).cuda())})
    net = make()
    rec.save("adm.frac", net, {"y": net(x, torch.tensor([12.5, 300.25]).cuda())})
    net = make(dims=1)
    rec.save("adm.dims1", net, {"y": net(torch.randn(2, 3, 16, generator=gen).cuda(), torch.tensor([40]).cuda())})
    net = make(dims=3)
    rec.save("adm.dims3", net, {"y": net(torch.randn(1, 3, 2, 16, 16, generator=gen).cuda(), torch.tensor([40]).cuda())})
    net = make(num_channels=128).bfloat16()
    rec.save("adm.bf16", net, {"y": net(x.bfloat16(), torch.tensor([40]).cuda())})
    meta, g = _golden("g5_adm_uncond")
    den = _adm(meta)
    smp = DDIMSampler(den, steps=2, silent=True)
    torch.manual_seed(22)
    x0 = smp(torch.randn(g["x"].shape, generator=gen).cuda())
    loop = next(iter(smp._fused_cache.values()))
    plans = {k: p for k, p in den.backbone._plans.items() if k[7] is not None}  # (the plan built with coef_ptr)
    assert plans, "the sampler did not take the fused loop"
    plans["loop"] = _LoopTape(loop.step_tapes[0], [loop, *plans.values()])
    rec.save("adm.fused_loop", den.backbone, {"x0": x0}, plans=plans)


def dit_cases(rec: Recorder) -> None:
    import torch

    from azula_amd.nn import DiT, DiTBlock, MultiheadSelfAttention, ViT

    pos44 = torch.cartesian_prod(torch.arange(4.0), torch.arange(4.0)).cuda()
    gen = torch.Generator().manual_seed(31)
    for name in ("g5_vit", "g5_vit_rope_swiglu", "g5_vit_relu2_noqknorm", "g24_vit_hd24"):
        meta, g = _golden(name)
        cfg = meta["cfg"]
        extra = {k: cfg[k] for k in ("rope", "ffn_activation", "qk_norm") if k in cfg}
        net = DiT(16, 16, pos_channels=2, mod_features=cfg["mod_features"], hid_channels=cfg["hid_channels"],
                  hid_blocks=cfg["hid_blocks"], attention_heads=cfg["attention_heads"], **extra)
        net.load_state_dict(_synth(meta))
        net = net.cuda().eval()
        x = torch.randn(2, 16, 16, generator=torch.Generator().manual_seed(51)).cuda()
        _fwd_vjp(rec, "dit." + name, net, x, g["modB"].cuda(), pos44)
        if name == "g5_vit":
            vit = ViT(cfg["in_channels"], cfg["out_channels"], hid_channels=cfg["hid_channels"], hid_blocks=cfg["hid_blocks"],
                      attention_heads=cfg["attention_heads"], patch_size=cfg["patch_size"], mod_features=cfg["mod_features"])
            vit.load_state_dict(_synth(meta))
            vit = vit.cuda().eval()
            rec.save("dit.vit_patch", vit, {"y": vit(g["x"].cuda(), g["modB"].cuda())})
            vit = vit.bfloat16()
            rec.save("dit.vit_bf16", vit, {"y": vit(g["x"].cuda().bfloat16(), g["modB"].cuda().bfloat16())})
    mask = torch.ones(9, 9, dtype=torch.bool).tril().cuda()
    pos33 = torch.cartesian_prod(torch.arange(3.0), torch.arange(3.0)).cuda()
    torch.manual_seed(32)
    msa = MultiheadSelfAttention(64, pos_channels=2, attention_heads=4, rope=True).cuda().eval()
    x = (torch.randn(2, 9, 64, generator=gen) * 2).cuda()
    _fwd_vjp(rec, "dit.msa_causal", msa, x, pos33, mask)
    torch.manual_seed(33)
    # ffn_factor 3 on 60 channels: a SwiGLU of width 180, not a multiple of 8 -> the pass of its own
    blk = DiTBlock(60, mod_features=32, ffn_factor=3, ffn_activation="swiglu", attention_heads=3).cuda().eval()
    x, mod = torch.randn(2, 9, 60, generator=gen).cuda(), torch.randn(2, 32, generator=gen).cuda()
    _fwd_vjp(rec, "dit.block_causal_swiglu_unfused", blk, x, mod, None, mask)


def jit_cases(rec: Recorder) -> None:
    import torch

    from azula_amd.plugins import jit

    t3 = torch.linspace(0.3, 0.8, 3)
    for name in ("g10_jit_ctx", "g10_jit_noctx_hd32", "g10_jit_hd80", "g24_jit_hd48"):
        meta, g = _golden(name)
        net = jit.JiT(**meta["cfg"])
        net.load_state_dict(_synth(meta))
        net = net.cuda().eval()
        x, y = g["x"].cuda(), g["y"].long().cuda()
        outs = {"y_shared": net(x, t3[1:2].cuda(), y), "y": net(x, t3.cuda(), y)}
        out, pull = net.vjp(x, t3.cuda(), y)
        outs.update(vjp_out=out, dx=pull(_cotangent(out)))
        rec.save("jit." + name, net, outs)
        if name == "g10_jit_ctx":
            net = net.bfloat16()
            rec.save("jit.bf16", net, {"y": net(x.bfloat16(), t3.cuda(), y)})


def sampler_cases(rec: Recorder) -> None:
    r"""Every step tape of the captured sampling loops and the sample they produce: each sampler on the fp32 clock and, where it
    takes the captured fp64 loop, with ``dtype=float64``.  Reads ``_fused_cache`` and ``step_tapes`` only, so the same file runs
    on an older checkout."""
    import torch

    from azula_amd import sample as S
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.guidance.repaint import RePaintSampler
    from azula_amd.nn import TimeModulated, UNet
    from azula_amd.noise import VPSchedule
    from oracle import synth

    net = TimeModulated(UNet(3, 3, hid_channels=(8, 16), hid_blocks=(1, 1), norm="group", groups=4, mod_features=16), 16, name="unet")
    net.load_state_dict(synth.synth_state_dict(synth.shapes_of(net.state_dict()), seed=42))
    den = KarrasDenoiser(net, VPSchedule()).cuda().eval()
    gen = torch.Generator().manual_seed(41)
    x1, y = torch.randn(2, 3, 16, 16, generator=gen).cuda(), torch.randn(2, 3, 16, 16, generator=gen).cuda()
    mask = (torch.rand(2, 1, 16, 16, generator=gen) < 0.5).cuda()
    cases = {  # name -> (class, arguments, takes the captured fp64 loop)
        "ddim_eta0": (S.DDIMSampler, {}, True), "ddim_eta05": (S.DDIMSampler, dict(eta=0.5), True), "ddpm": (S.DDPMSampler, {}, True),
        "euler": (S.EulerSampler, {}, True), "heun": (S.HeunSampler, {}, True), "ito_eta07": (S.ItoSampler, dict(eta=0.7), True),
        "pc_2": (S.PCSampler, dict(corrections=2), True), "zab_3": (S.zABSampler, dict(order=3), True),
        "repaint_2": (RePaintSampler, dict(y=y, mask=mask, iterations=2), False),
    }
    for name, (cls, kw, wide) in cases.items():
        for clock, dtype in (("f32", None), ("f64", torch.float64))[: 2 if wide else 1]:
            smp = cls(den, steps=5, silent=True, dtype=dtype, **kw)
            torch.manual_seed(43)
            x0 = smp(x1)
            loop = next(iter(smp._fused_cache.values()), None)
            assert hasattr(loop, "step_tapes"), f"{name} on the {clock} clock did not take the captured loop"
            assert x0.dtype == (torch.float64 if dtype else torch.float32)
            roots = [loop, *(m._plans for m in den.modules() if hasattr(m, "_plans"))]
            plans = {j: _LoopTape(t, roots) for j, t in enumerate(loop.step_tapes)}
            # (an fp64 sample as pairs of fp32 words: the recorder stores fp32, and the comparison is of bits)
            rec.save(f"samplers.{name}.{clock}", den, {"x0": x0.view(torch.float32)}, plans=plans)


def _two_step_loop(rec: Recorder, case: str, den, backbone, x1) -> None:
    r"""A two-step DDIM sample on the captured loop: every plan the backbone holds afterwards (the sampler's own among them) and
    every step tape."""
    import torch

    from azula_amd.sample import DDIMSampler

    smp = DDIMSampler(den, steps=2, silent=True)
    torch.manual_seed(44)
    x0 = smp(x1)
    loop = next(iter(smp._fused_cache.values()), None)
    assert hasattr(loop, "step_tapes"), f"{case}: the sampler did not take the captured loop"
    plans = dict(backbone._plans)
    roots = [loop, *plans.values()]
    plans.update({f"step{j}": _LoopTape(t, roots) for j, t in enumerate(loop.step_tapes)})
    rec.save(case, backbone, {"x0": x0}, plans=plans)


def vdm_cases(rec: Recorder) -> None:
    r"""Narrow v-diffusion backbones: ``skip_main`` concatenation with nearest up-sampling (imagenet_128, five poolings: 32 x 32)
    and ``main_skip`` with bilinear up-sampling (yfcc_1, seven poolings: 128 x 128 is its smallest map), then the ``coef_ptr`` plan
    of the first under a two-step sampler."""
    import torch

    from azula_amd.plugins.vdm import VelocityDenoiser
    from azula_amd.plugins.vdm.model import VDMModel

    gen = torch.Generator().manual_seed(61)
    for name, model, c, shape in (("nearest", "imagenet_128", 32, (2, 3, 32, 32)), ("bilinear", "yfcc_1", 16, (1, 3, 128, 128))):
        torch.manual_seed(62)
        net = VDMModel(model, base_channels=c)
        _randomise(net, 63)
        net = net.cuda().eval()
        x = torch.randn(shape, generator=gen).cuda()
        rec.save("vdm." + name, net, {"y": net(x, torch.tensor([0.3, 0.8][: shape[0]]).cuda())})
        if name == "nearest":
            net._plans.clear()
            _two_step_loop(rec, "vdm.fused_loop", VelocityDenoiser(net).cuda().eval(), net, x)


def _time_modulated(net, name: str):
    from azula_amd.denoise import KarrasDenoiser
    from azula_amd.nn import TimeModulated
    from azula_amd.noise import VPSchedule

    _randomise(net, 73)
    return KarrasDenoiser(TimeModulated(net, 16, name=name), VPSchedule()).cuda().eval()


def unet3d_cases(rec: Recorder) -> None:
    import torch

    from azula_amd.nn import UNet

    gen = torch.Generator().manual_seed(71)
    torch.manual_seed(72)
    net = UNet(3, 3, hid_channels=(8, 16), hid_blocks=(1, 1), norm="group", groups=4, mod_features=16, spatial=3)
    den = _time_modulated(net, "unet")
    x, mod = torch.randn(1, 3, 4, 8, 8, generator=gen).cuda(), torch.randn(1, 16, generator=gen).cuda()
    rec.save("unet3d.forward", net, {"y": net(x, mod)})
    net._plans.clear()
    _two_step_loop(rec, "unet3d.fused_loop", den, net, x)


def vit_fused_cases(rec: Recorder) -> None:
    import torch

    from azula_amd.nn import ViT

    gen = torch.Generator().manual_seed(81)
    torch.manual_seed(82)
    net = ViT(3, 3, hid_channels=64, hid_blocks=2, attention_heads=4, patch_size=4, mod_features=16)
    den = _time_modulated(net, "vit")
    _two_step_loop(rec, "vit.fused", den, net, torch.randn(2, 3, 16, 16, generator=gen).cuda())


CASES = {"unet": unet_cases, "adm": adm_cases, "dit": dit_cases, "jit": jit_cases, "samplers": sampler_cases, "vdm": vdm_cases,
         "unet3d": unet3d_cases, "vit.fused": vit_fused_cases}


def run(out_dir: str, only: list[str]) -> None:
    import torch

    sys.path.insert(0, ROOT)
    torch.set_grad_enabled(False)
    rec = Recorder(out_dir)
    for name in only:
        CASES[name](rec)
    torch.cuda.synchronize()
    print(f"{len(rec.index)} cases written to {out_dir}")


# ------------------------------------------------------------------------------------------------ comparison
def compare(dir_a: str, dir_b: str) -> int:
    r"""One line per case: signatures (equal / pool placement only / DIFFERENT) and outputs (bit-equal or not).  Exit status 1
    when a signature differs by more than pool placement on a gradient tape, or a case is missing."""
    import numpy as np

    bad = 0
    cases = sorted(f[:-5] for f in os.listdir(dir_a) if f.endswith(".json"))
    for case in cases:
        path_b = os.path.join(dir_b, case + ".json")
        if not os.path.exists(path_b):
            print(f"{case}: MISSING in {dir_b}")
            bad += 1
            continue
        a, b = (json.load(open(os.path.join(d, case + ".json"))) for d in (dir_a, dir_b))
        notes = []
        if sorted(a) != sorted(b):
            notes.append(f"plans {sorted(a)} vs {sorted(b)}")
            bad += 1
        for plan in sorted(set(a) & set(b)):
            for tape in ("tape", "fwd", "bwd"):
                if tape not in a[plan]:
                    continue
                sa, sb = a[plan][tape], b[plan][tape]
                if sa == sb:
                    continue
                ma = mask_ordinals(sa, set(a[plan][tape + "_pool_ordinals"]))
                mb = mask_ordinals(sb, set(b[plan][tape + "_pool_ordinals"]))
                grew = b[plan].get("saved_bytes", 0) > a[plan].get("saved_bytes", 0)
                if tape != "tape" and ma == mb and not grew:
                    notes.append(f"{plan}.{tape}: pool placement differs (saved_bytes {a[plan]['saved_bytes']} -> {b[plan]['saved_bytes']})")
                else:
                    at = next((i for i, (x, y) in enumerate(zip(sa, sb)) if x != y), min(len(sa), len(sb)))
                    notes.append(f"{plan}.{tape}: DIFFERENT at op {at} of {len(sa)} / {len(sb)}"
                                 f" ({sa[at][0] if at < len(sa) else '-'} / {sb[at][0] if at < len(sb) else '-'})")
                    bad += 1
        outs = sorted(f for f in os.listdir(dir_a) if f.startswith(case + ".") and f.endswith(".npy"))
        unequal = [f[len(case) + 1 : -4] for f in outs
                   if not os.path.exists(os.path.join(dir_b, f))
                   or np.load(os.path.join(dir_a, f)).tobytes() != np.load(os.path.join(dir_b, f)).tobytes()]
        print(f"{case}: signatures {'; '.join(notes) if notes else 'equal'}; outputs "
              f"{'bit-equal' if not unequal else 'DIFFER: ' + ', '.join(unequal)} ({len(outs)})")
    print(f"{len(cases)} cases, {bad} signature failures")
    return 1 if bad else 0


def main(argv: list[str]) -> int:
    if len(argv) >= 2 and argv[0] == "run":
        only = list(CASES)
        if "--only" in argv:
            only = argv[argv.index("--only") + 1].split(",")
        run(argv[1], only)
        return 0
    if len(argv) == 3 and argv[0] == "compare":
        return compare(argv[1], argv[2])
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
