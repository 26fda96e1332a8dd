"""Helpers for the -m gpu parity tests: every call goes through the C ABI of libhwocr_hip.so."""
import torch

from handwritten_ocr_amd import _lib

DEV = "cuda"


def lib():
    return _lib.hip()


def p(t):
    return _lib.ptr(t)


def st():
    return _lib.stream_handle()


def rbf(x: torch.Tensor) -> torch.Tensor:
    """fp32 value after a round trip through bf16 (a materialised bf16 tensor in the reference's modules)."""
    return x.to(torch.bfloat16).to(torch.float32)


def randbf(*shape, scale=1.0, seed=None):
    g = torch.Generator(device="cpu")
    g.manual_seed(0 if seed is None else seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


def randf32(*shape, seed=0):
    """fp32 N(0, 1) on the device from a SEEDED host generator: a test's data must not depend on which tests ran before it (the device
    RNG's state does; round 4: an unseeded torch.randn(..., device=...) made test_add_rmsnorm's data, and with it a one-in-a-million
    rounding coincidence, a function of the test order)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def assert_close_bf16(got: torch.Tensor, want_f32: torch.Tensor, ulps: float = 2.0, atol: float = 1e-3, what="",
                      mag: torch.Tensor | None = None):
    """got: bf16 kernel output; want: fp32 reference.  1 bf16 ulp of x = 2^(floor(log2|x|) - 7).
    `mag` (optional) is the magnitude the ulp is taken of when a larger rounded intermediate feeds the output."""
    g = got.float()
    err = (g - want_f32).abs()
    ref_mag = want_f32.abs() if mag is None else torch.maximum(want_f32.abs(), mag)
    ulp = torch.exp2(torch.floor(torch.log2(ref_mag.clamp_min(1e-30))) - 7.0)
    tol = atol + ulps * ulp
    bad = err > tol
    assert not bad.any(), (
        f"{what}: {int(bad.sum())}/{bad.numel()} elements off; max err {float(err.max()):.4g} "
        f"at ref {float(want_f32.flatten()[err.argmax()]):.4g}")


def bf16_neighbours(x: torch.Tensor) -> torch.Tensor:
    """[..., 3]: a bf16-representable fp32 value with its two bf16 neighbours (one ulp down / up in the bit pattern)."""
    b = x.to(torch.bfloat16).view(torch.int16)
    return torch.stack([(b - 1).view(torch.bfloat16).float(), x.float(), (b + 1).view(torch.bfloat16).float()], dim=-1)


def assert_close_bf16_explained(got: torch.Tensor, want_f32: torch.Tensor, ulps: float, atol: float, what: str, mag, candidates,
                                max_frac: float = 4e-6):
    """As assert_close_bf16 with `ulps` as the hard bound for ALL BUT a vanishing share of the outputs — and every element beyond it
    must be EXPLAINED: an epilogue with several rounding points (bf16(acc + bias), a rounded gate or activation, the output) can
    legitimately land further out when the kernel's fp32 accumulator (another summation order than the reference product's) sits on
    the other side of a rounding boundary at more than one of them at once.  `candidates(flat_idx) -> [n, c]` recomputes the epilogue
    from the REFERENCE accumulator at those elements with each rounded intermediate moved by -1 / 0 / +1 ulp; the kernel's output
    must be the bf16 rounding of one of these outcomes (within 0.5 ulp of it, + 2 % of an ulp for the fp32 transcendental).  An
    indexing slip, a wrong operand or a dropped K tile does not produce a value one rounding flip away from the reference, so such
    outliers fail here whatever their count — that is the test; the count bound behind it only says "rare".  Expected share, order
    of magnitude: P(bf16(acc + bias) flips) ~ accumulation noise / bf16 spacing ~ 1e-6 / 2^-8 = 2.5e-4, x P(the rounded gate then
    flips too) ~ 0.3, x P(both land on the far side of the output's rounding) ~ 2 % = 1.5e-6.  Measured (round 4, first run of
    this rule): bf16 GEMMs 12 of 3.2e8 = 4e-8; the E4M3 GEMM, whose 128-long MFMA dot products carry more accumulation noise, 98 of
    8.0e7 = 1.2e-6, every one of them explained.  Returns the number of explained outliers."""
    g = got.float()
    err = (g - want_f32).abs()
    ref_mag = want_f32.abs() if mag is None else torch.maximum(want_f32.abs(), mag)
    ulp = torch.exp2(torch.floor(torch.log2(ref_mag.clamp_min(1e-30))) - 7.0)
    bad = (err > atol + ulps * ulp).flatten()
    n_bad = int(bad.sum())
    if n_bad == 0:
        return 0
    # the count floor scales with the output: below 1 / max_frac elements (250 000 at the default) not one element may pass the hard
    # bound, explained or not — a small output has no room for "rare" coincidences
    limit = int(max_frac * bad.numel())
    assert n_bad <= max(64 * limit, 256), f"{what}: {n_bad}/{bad.numel()} elements beyond {ulps} ulps; max err {float(err.max()):.4g}"
    idx = bad.nonzero().flatten()
    cand = candidates(idx)                                              # [n, c] fp32
    gv = g.flatten()[idx].unsqueeze(1)
    culp = torch.exp2(torch.floor(torch.log2(cand.abs().clamp_min(1e-30))) - 7.0)
    ok = ((gv - cand).abs() <= 0.52 * culp + 1e-6).any(dim=1)
    assert bool(ok.all()), (f"{what}: {int((~ok).sum())} of {n_bad} elements beyond {ulps} ulps are NOT one rounding flip away from the "
                            f"reference: got {gv[~ok].flatten()[:4].tolist()}, want {want_f32.flatten()[idx][~ok][:4].tolist()}")
    assert n_bad <= limit, (f"{what}: {n_bad}/{bad.numel()} elements beyond {ulps} ulps (more than {limit}: each is one rounding flip "
                            f"away from the reference, but that many are not rare coincidences); max err {float(err.max()):.4g}")
    return n_bad


def _k_offsets(ctx):
    key = torch.arange(ctx).view(-1, 1)
    d = torch.arange(128).view(1, -1)
    kl = key & 31
    t = (kl >> 2) & 1
    c = ((kl >> 3) << 2) | (kl & 3)
    return (((((key >> 5) * 2 + t) * 4 + (d >> 5)) * 64 + ((d >> 3) & 3) * 16 + c) * 8 + (d & 7)).reshape(-1)


def _v_offsets(ctx):
    d = torch.arange(128).view(-1, 1)
    key = torch.arange(ctx).view(1, -1)
    kl = key & 31
    return ((((key >> 5) * 8 + (d >> 4)) * 64 + (kl >> 3) * 16 + (d & 15)) * 8 + (kl & 7)).reshape(-1)


def tile_k(k):
    """[..., ctx, 128] row-major -> the fragment-tiled cache order (csrc/common.h kv_tiled_k), same shape."""
    ctx = k.shape[-2]
    out = torch.empty_like(k).view(*k.shape[:-2], ctx * 128)
    out[..., _k_offsets(ctx).to(k.device)] = k.reshape(*k.shape[:-2], ctx * 128)
    return out.view(k.shape)


def untile_k(t):
    ctx = t.shape[-2]
    return t.reshape(*t.shape[:-2], ctx * 128)[..., _k_offsets(ctx).to(t.device)].view(t.shape)


def tile_v(vt):
    """[..., 128, ctx] row-major -> fragment-tiled (kv_tiled_v)."""
    ctx = vt.shape[-1]
    out = torch.empty_like(vt).view(*vt.shape[:-2], ctx * 128)
    out[..., _v_offsets(ctx).to(vt.device)] = vt.reshape(*vt.shape[:-2], ctx * 128)
    return out.view(vt.shape)


def untile_v(t):
    ctx = t.shape[-1]
    return t.reshape(*t.shape[:-2], ctx * 128)[..., _v_offsets(ctx).to(t.device)].view(t.shape)
