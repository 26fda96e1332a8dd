"""Kernel parity at the VALUES real checkpoints produce, not only at N(0, 1) operands: the rest of the operator suite draws almost every
operand from randbf (Gaussian times ~K^-0.5), so paths that only matter away from |x| ~ 1 are driven here.
  * attention under a dominant key: a sink logit 30-80 above the rest at position 0 or in the LAST key tile / split (every earlier
    partial rescaled by ~1e-13 .. 1e-35), two equal maxima in different splits, every score shifted by -200 (float64 softmax reference)
  * GEMM epilogue tails: pre-activations from ~1e-3 to past the fp32 exp overflow (|t| > 88.7) and a row past the x^3 overflow
  * norms over rows with outlier channels (1e3-1e4 over N(0, 1): an ASSUMED magnitude, not measured on a checkpoint), constant rows,
    rows whose variance is below eps, a ~1e4 residual with a ~1e-2 update
  * every finite E4M3 code through the fp8 GEMM, the decode attention over the E4M3 cache and all four quantisers (codes, rounding ties)
  * the E4M3 KV cache against bf16 attention on the unquantised K / V, under a rigorous float64 bound (tests/_ranges.kv8_error_bound)
Operands come from seeded host generators; tolerances are the suite's existing ones, written at each assert."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fp8_ref  # noqa: E402
from tests import test_kv_fp8_128_gpu as kv128, test_kv_fp8_gpu as kv256  # noqa: E402
from tests._gpu_util import (DEV, assert_close_bf16, assert_close_bf16_explained, bf16_neighbours, lib, p, randbf,  # noqa: E402
                             randf32, rbf, st, tile_k, tile_v)
from tests._ranges import coverage_codes, e4m3_finite_codes, e4m3_quant_pool, kv8_error_bound, row_scales  # noqa: E402
from tests.test_ops_gpu import (_check_epilogue, _check_gated, _fp8_gemm_ref, _rope_tables, _sdpa_ref, _tiled,  # noqa: E402
                                _rows16_norm_ref)


def sync():
    torch.cuda.synchronize()


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ------------------------------------------------------------------------------------------------ attention with large logits
# Every query carries A on feature 0 and every key 0 there, so feature 0 adds exactly A * c * scale to a key's score when the key
# holds c: a planted key's scaled logit sits `L` above the N(0, 1)-spread rest, for every query at once.  Scenarios:
#   first  L   the sink at key 0 (the running max is set by the first tile and never moves)
#   last   L   the sink in the last key tile / split: every earlier partial must be rescaled by alpha = e^-L (1e-13 .. 1e-35)
#   two    L   two identical sink keys, at 0 and in the last tile / split: equal maxima, the output is the mean of their values
#   shift      every key -200: all scores strongly negative; the softmax (float64) and the output are those of the unshifted case
A = 8.0
#   (last 100: past e^88.7, so a partial referenced to any maximum but the true one overflows fp32)
SCENARIOS = [("first", 80.0), ("last", 30.0), ("last", 80.0), ("last", 100.0), ("two", 30.0)]


def _plant(q, k, lens, scale, kind, L, key_axis, late=None):
    """q [..., d] and k [..., keys, d] (keys on `key_axis` of k's segment view) modified in place per segment / read."""
    q[..., 0] = A
    k[..., 0] = 0.0
    c = float(torch.tensor(L / (A * scale)).to(torch.bfloat16))
    for s, n in enumerate(lens):
        ks = k[s]
        j_late = (n - 1) if late is None else late(n)
        if kind == "shift":
            ks.narrow(key_axis, 0, n)[..., 0] = float(torch.tensor(-200.0 / (A * scale)).to(torch.bfloat16))
            continue
        if kind in ("last", "two"):
            ks.narrow(key_axis, j_late, 1)[..., 0] = c
        if kind in ("first", "two"):
            ks.narrow(key_axis, 0, 1)[..., 0] = c
        if kind == "two" and j_late != 0:
            ks.narrow(key_axis, j_late, 1).copy_(ks.narrow(key_axis, 0, 1))


def _prefill(q, k, vt, lens, Hq, Hkv, hd, causal, tiled, Lp):
    """hwocr_attn_prefill, head-major layout: q [nseg][Hq][Lp][hd], k [nseg][Hkv][Lp][hd], vt [nseg][Hkv][hd][Lp] -> [nseg][Lp][Hq*hd]."""
    nseg = len(lens)
    out = torch.zeros(nseg, Lp, Hq * hd, dtype=torch.bfloat16, device=DEV)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kk, vv = (tile_k(k), tile_v(vt)) if tiled else (k, vt)
    vbuf = torch.zeros(vv.numel() + 64, dtype=torch.bfloat16, device=DEV)     # 64 elements of slack past V^T, as the ABI asks
    vbuf[: vv.numel()] = vv.reshape(-1)
    rc = lib().hwocr_attn_prefill(p(q), p(kk), p(vbuf), p(out), p(lens_d), nseg, Hq, Hq // Hkv, hd, max(lens), int(causal),
                                  Hq * Lp * hd, Lp * hd, hd, Hkv * Lp * hd, Lp * hd, hd, Hkv * hd * Lp, hd * Lp, Lp,
                                  Lp * Hq * hd, Hq * hd, hd ** -0.5, tiled, st())
    assert rc == 0
    sync()
    return out


def _prefill_case(hd, Hq, Hkv, causal, tiled, lens, Lp, kind, L, seed):
    scale = hd ** -0.5
    nseg = len(lens)
    q = randbf(nseg, Hq, Lp, hd, seed=seed)
    k = randbf(nseg, Hkv, Lp, hd, seed=seed + 1)
    v = randbf(nseg, Hkv, Lp, hd, seed=seed + 2)
    # causal: the late sink at 7/8 of the segment, so that the queries past it have walked earlier tiles first
    _plant(q, k, lens, scale, kind, L, key_axis=1, late=(lambda n: (7 * n) // 8) if causal else None)
    vt = v.transpose(2, 3).contiguous()
    for s, n in enumerate(lens):                                 # key padding poisoned: it must never reach the output
        vt[s, :, :, n:] = float("nan")
        k[s, :, n:, :] = 1e4
    out = _prefill(q, k, vt, lens, Hq, Hkv, hd, causal, tiled, Lp)
    for s, n in enumerate(lens):
        want = _sdpa_ref(q[s, :, :n].double(), k[s, :, :n].double(), v[s, :, :n].double(), causal, scale).float()
        got = out[s, :n].view(n, Hq, hd)
        assert torch.isfinite(got.float()).all(), f"{kind} {L}: non-finite output in segment {s}"
        # P rounded to bf16 before the PV product, as in test_attn_prefill: 4 output ulps + 4e-3
        assert_close_bf16(got, want, ulps=4.0, atol=4e-3, what=f"attn_prefill hd {hd} {kind} {L} seg {s}")
    return out


# (hd, Hq, Hkv, causal, tiled): the `small` tower heads, the ViT-80 heads, the decoder's 128 (tiled cache, GQA), Gemma's 256
PREFILL_RANGE_CASES = [(64, 2, 1, True, 0), (64, 4, 4, False, 0), (80, 4, 4, False, 0), (128, 6, 2, True, 1), (128, 2, 2, False, 0),
                       (256, 4, 1, False, 0), (256, 2, 1, True, 0)]
PREFILL_LENS, PREFILL_LP = [300, 64, 37, 129], 320


@pytest.mark.parametrize("kind,L", SCENARIOS)
@pytest.mark.parametrize("hd,Hq,Hkv,causal,tiled", PREFILL_RANGE_CASES)
def test_attn_prefill_dominant_key(hd, Hq, Hkv, causal, tiled, kind, L):
    _prefill_case(hd, Hq, Hkv, causal, tiled, PREFILL_LENS, PREFILL_LP, kind, L, seed=300)


@pytest.mark.parametrize("hd,Hq,Hkv,causal,tiled", PREFILL_RANGE_CASES)
def test_attn_prefill_shift_invariance(hd, Hq, Hkv, causal, tiled):
    """Every score moved by -200: the same output as unshifted (the float64 softmax of both is identical), finite."""
    base = _prefill_case(hd, Hq, Hkv, causal, tiled, PREFILL_LENS, PREFILL_LP, "none", 0.0, seed=310)
    shifted = _prefill_case(hd, Hq, Hkv, causal, tiled, PREFILL_LENS, PREFILL_LP, "shift", 0.0, seed=310)
    for s, n in enumerate(PREFILL_LENS):
        assert_close_bf16(shifted[s, :n], base[s, :n].float(), ulps=4.0, atol=4e-3, what=f"shifted vs unshifted seg {s}")


VIT80_LENS = [2000, 1537, 383, 769]


@pytest.mark.parametrize("kind,L", SCENARIOS + [("shift", 0.0)])
@pytest.mark.parametrize("kernel", ["x", "12", "4"])
def test_attn_vit80_dominant_key(kernel, kind, L, monkeypatch):
    """The three forms of the head_dim-80 kernel (HWOCR_VIT80_KERNEL) on page-length segments: their lazy running maximum (rescale
    only past `slack`) must still rescale for a sink 30-80 above the rest in the last tile, and take a -200 shift."""
    monkeypatch.setenv("HWOCR_VIT80_KERNEL", kernel)
    _prefill_case(80, 2, 2, False, 0, VIT80_LENS, 2048, kind, L, seed=320)


@pytest.mark.parametrize("kind,L", SCENARIOS + [("shift", 0.0)])
def test_attn_varlen_dominant_key(kind, L):
    """Packed ragged windows (Qwen2.5-VL windowed layers), planted keys in every window."""
    hd, heads = 80, 4
    lens = [64, 16, 32, 4, 64, 36, 8, 48, 12, 64]
    offs = [sum(lens[:i]) for i in range(len(lens))]
    rows = 384
    scale = hd ** -0.5
    q = randbf(heads, rows, hd, seed=331)
    k = randbf(heads, rows, hd, seed=332)
    v = randbf(heads, rows, hd, seed=333)
    # plant per window: view each window as a segment [heads][n][hd]
    q[..., 0] = A
    k[..., 0] = 0.0
    for o, n in zip(offs, lens):
        _plant(q[:, o: o + n].unsqueeze(0), k[:, o: o + n].unsqueeze(0), [n], scale, kind, L, key_axis=1)   # views: k is planted in place
    vt = torch.zeros(heads * hd * rows + 64, dtype=torch.bfloat16, device=DEV)
    vt[: heads * hd * rows] = v.transpose(1, 2).reshape(-1)
    out = torch.zeros(rows, heads * hd, dtype=torch.bfloat16, device=DEV)
    off_d = torch.tensor(offs, dtype=torch.int32, device=DEV)
    len_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    assert lib().hwocr_attn_varlen(p(q), p(k), p(vt), p(out), p(off_d), p(len_d), len(lens), heads, hd, max(lens),
                                   rows * hd, hd, rows * hd, hd, hd * rows, rows, heads * hd, scale, st()) == 0
    sync()
    for o, n in zip(offs, lens):
        want = _sdpa_ref(q[:, o: o + n].double(), k[:, o: o + n].double(), v[:, o: o + n].double(), False, scale).float()
        got = out[o: o + n].view(n, heads, hd)
        assert torch.isfinite(got.float()).all()
        assert_close_bf16(got, want, ulps=4.0, atol=4e-3, what=f"attn_varlen {kind} {L} window at {o}")


def _decode(q, kk, vv, lens, Hq, Hkv, hd, ctx, nsplit, tiled, arrive):
    B = len(lens)
    G = Hq // Hkv
    out = torch.full((B, Hq * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    part_o = torch.full((B * Hkv * nsplit * G * hd,), float("nan"), dtype=torch.float32, device=DEV)
    part_ml = torch.full((B * Hkv * nsplit * G * 2,), float("nan"), dtype=torch.float32, device=DEV)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    rc = lib().hwocr_attn_decode(p(q), p(kk), p(vv), p(lens_d), p(out), p(part_o), p(part_ml), p(arrive) if arrive is not None else None,
                                 B, Hq, Hkv, nsplit, Hkv * ctx * hd, ctx * hd, Hkv * hd * ctx, hd * ctx, ctx, hd ** -0.5, hd, tiled, st())
    assert rc == 0
    sync()
    return out


DECODE_LENS, DECODE_CTX = [1024, 700, 2, 333, 65], 1024


@pytest.mark.parametrize("kind,L", SCENARIOS + [("shift", 0.0)])
@pytest.mark.parametrize("nsplit", [1, 4, 16])
@pytest.mark.parametrize("hd,Hq,Hkv,tiled", [(128, 12, 2, 0), (128, 12, 2, 1), (256, 8, 1, 0)])
def test_attn_decode_dominant_key(hd, Hq, Hkv, tiled, nsplit, kind, L):
    """hwocr_attn_decode (rows and tiled layouts) at 1 / 4 / 16 splits: the late sink sits in the LAST split of the long reads, so the
    merge (launch and last-arriving workgroup alike) must rescale every other split's partial by e^-L; "two" puts equal maxima in the
    first and last splits.  Against the float64 softmax."""
    lens, ctx = DECODE_LENS, DECODE_CTX
    B, scale = len(lens), hd ** -0.5
    q = randbf(B, Hq, hd, seed=340)
    k = randbf(B, Hkv, ctx, hd, seed=341)
    v = randbf(B, Hkv, ctx, hd, seed=342)
    _plant(q, k, lens, scale, kind, L, key_axis=1)
    vt = v.transpose(2, 3).contiguous()
    for b, n in enumerate(lens):
        vt[b, :, :, n:] = float("nan")
        k[b, :, n:, :] = 1e4
    kk, vv = (tile_k(k), tile_v(vt)) if tiled else (k, vt)
    outs = [_decode(q, kk, vv, lens, Hq, Hkv, hd, ctx, nsplit, tiled, None)]
    if nsplit > 1:
        arrive = torch.zeros(B * Hkv, dtype=torch.int32, device=DEV)
        outs.append(_decode(q, kk, vv, lens, Hq, Hkv, hd, ctx, nsplit, tiled, arrive))
        assert int(arrive.abs().sum()) == 0
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "last-workgroup merge differs from the merge launch"
    for b, n in enumerate(lens):
        want = _sdpa_ref(q[b].double().unsqueeze(1), k[b, :, :n].double(), v[b, :, :n].double(), False, scale).reshape(Hq * hd).float()
        assert torch.isfinite(outs[0][b].float()).all(), f"{kind} {L}: non-finite output, read {b}"
        assert_close_bf16(outs[0][b], want, ulps=4.0, atol=4e-3, what=f"attn_decode {kind} {L} nsplit {nsplit} read {b} len {n}")
    if kind == "shift":
        qb, kb, vb = randbf(B, Hq, hd, seed=340), randbf(B, Hkv, ctx, hd, seed=341), randbf(B, Hkv, ctx, hd, seed=342)
        _plant(qb, kb, lens, scale, "none", 0.0, key_axis=1)
        vbt = vb.transpose(2, 3).contiguous()
        for b, n in enumerate(lens):
            vbt[b, :, :, n:] = float("nan")
            kb[b, :, n:, :] = 1e4
        base = _decode(qb, *((tile_k(kb), tile_v(vbt)) if tiled else (kb, vbt)), lens, Hq, Hkv, hd, ctx, nsplit, tiled, None)
        assert_close_bf16(outs[0], base.float(), ulps=4.0, atol=4e-3, what="decode: shifted vs unshifted")


# ------------------------------------------------------------------------------------------------ GEMM epilogue tails
# Rows of X scaled so that the pre-activations sweep ~1e-3 .. ~160 in magnitude (past the fp32 exp overflow at |t| = 88.7), plus a
# row at ~1e5 and one at ~1e13 (past the x^3 overflow of the tanh GELU's cubic at 7e12).  Beyond the explained-outlier rule on every
# element, the saturated ends are pinned exactly:
#   * x >= 30: the activation IS x (sigmoid(>= 30) == 1 in fp32): the output is bf16(x) of the kernel's own x = bf16(acc + bias),
#     i.e. bf16(x) or one of its neighbours;
#   * deep negative (quick-GELU x < -60: exp(-1.702 x) overflows; tanh GELU x < -15: exp(-2u) overflows; erf GELU x < -12:
#     1 + erf(x / sqrt 2) == 0 in fp32): the output is exactly +-0, as the fp32 reference's (the exact value is below 1e-36).
TAIL_DEEP = {2: -60.0, 3: -12.0, 6: -15.0}
GATE_DEEP = {False: -100.0, True: -15.0}   # SiLU: exp(-g) overflows; GeGLU: as the tanh GELU


def _tail_x(M, K, seed):
    g = _gen(seed)
    s = torch.cat([row_scales(M - 2, 1e-3, 40.0, g), torch.tensor([1e5, 1e13])])
    x = torch.randn(M, K, generator=g) * s[:, None]
    return x.to(torch.bfloat16).to(DEV)


def _check_tails(out, x_ref, deep, what):
    """out: the kernel's bf16 output; x_ref: bf16(acc + bias) of the reference accumulator."""
    o = out.float()
    assert torch.isfinite(o).all(), f"{what}: non-finite output"
    big = x_ref >= 30.0
    nb = bf16_neighbours(x_ref[big])                                           # [n, 3]
    assert bool((o[big].unsqueeze(-1) == nb).any(-1).all()), f"{what}: a large positive input does not return x"
    dn = x_ref < deep
    assert int(dn.sum()) > 0 and int(big.sum()) > 0, "the sweep must reach both saturated ends"
    assert bool((o[dn] == 0).all()), f"{what}: a deep negative input returns {o[dn][o[dn] != 0][:4].tolist()}, not +-0"


def _check_gated_tails(out, acc, geglu, what):
    M, N = acc.shape
    a = acc.view(M, N // 32, 2, 16)
    g, u = rbf(a[:, :, 0, :].reshape(M, N // 2)), rbf(a[:, :, 1, :].reshape(M, N // 2))
    o = out.float()
    assert torch.isfinite(o).all(), f"{what}: non-finite output"
    big = g >= 30.0                                       # act(g) == g: out = bf16(g' u') for the kernel's own rounded g', u'
    cand = rbf(bf16_neighbours(g[big]).unsqueeze(-1) * bf16_neighbours(u[big]).unsqueeze(-2)).flatten(1)
    assert bool((o[big].unsqueeze(-1) == cand).any(-1).all()), f"{what}: a large positive gate does not return gate x up"
    dn = g < GATE_DEEP[geglu]
    assert int(dn.sum()) > 0 and int(big.sum()) > 0, "the sweep must reach both saturated ends"
    assert bool((o[dn] == 0).all()), f"{what}: a deep negative gate returns {o[dn][o[dn] != 0][:4].tolist()}, not +-0"


# (M, N, K): the 128 x 128 kernel (M < 1024) and the 256 x 256 one
TAIL_SHAPES = [(320, 256, 256), (1024, 512, 256)]


@pytest.mark.parametrize("epi", [2, 3, 6])
@pytest.mark.parametrize("M,N,K", TAIL_SHAPES)
def test_gemm_wide_activation_tails(M, N, K, epi):
    x = _tail_x(M, K, seed=400)
    w = randbf(N, K, scale=K ** -0.5, seed=401)
    bias = randbf(N, scale=0.5, seed=402)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert lib().hwocr_gemm_wide(p(x), p(w), p(bias), None, p(out), M, N, K, K, K, N, N, epi, st()) == 0
    sync()
    acc = x.float() @ w.float().t()
    what = f"gemm_wide tails epi={epi} {M}x{N}x{K}"
    _check_tails(out, rbf(acc + bias.float()), TAIL_DEEP[epi], what)
    _check_epilogue(out, acc, bias, None, epi, what)            # 2 ulps + 2e-3; explained outliers only


@pytest.mark.parametrize("geglu", [False, True])
@pytest.mark.parametrize("M,N,K", [(320, 512, 256), (1024, 1024, 256)])
def test_gemm_wide_gated_tails(M, N, K, geglu):
    x = _tail_x(M, K, seed=410)
    w = randbf(N, K, scale=K ** -0.5, seed=411)
    out = torch.full((M, N // 2), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert lib().hwocr_gemm_wide(p(x), p(w), None, None, p(out), M, N, K, K, K, N // 2, 0, 7 if geglu else 4, st()) == 0
    sync()
    acc = x.float() @ w.float().t()
    what = f"gemm_wide gated tails geglu={geglu} {M}x{N}x{K}"
    _check_gated_tails(out, acc, geglu, what)
    _check_gated(out, acc, None, geglu, what)


@pytest.mark.parametrize("geglu", [False, True])
@pytest.mark.parametrize("kernel,B", [("skinny", 48), ("rows16", 7)])
def test_gemm_decode_gated_tails(kernel, B, geglu):
    """The decode step's gate/up GEMM (tiled weights): hwocr_gemm_skinny at 48 reads, hwocr_gemm_rows16 at 7."""
    N, K = 2 * 1792, 1536
    x = _tail_x(B, K, seed=420)
    w = randbf(N, K, scale=K ** -0.5, seed=421)
    wk = _tiled(w)
    epi = 7 if geglu else 4
    out = torch.full((B, N // 2), float("nan"), dtype=torch.bfloat16, device=DEV)
    if kernel == "skinny":
        assert lib().hwocr_gemm_skinny(p(x), p(wk), None, p(out), B, N, K, K, K, N // 2, epi, 1, 1, st()) == 0
    else:
        assert lib().hwocr_gemm_rows16(p(x), K, p(wk), p(out), N // 2, B, N, K, epi, 1, None, st()) == 0
    sync()
    acc = x.float() @ w.float().t()
    what = f"{kernel} gated tails geglu={geglu}"
    _check_gated_tails(out, acc, geglu, what)
    _check_gated(out, acc, None, geglu, what)


# ------------------------------------------------------------------------------------------------ norms: outlier channels, flat rows
def _norm_rows(rows, D, seed):
    """bf16 rows, cycling through: N(0, 1.5); N(0, 1) with 2-4 channels at +-1e3 .. 1e4 (outliers, ASSUMED magnitudes); a constant row
    (3, -7.5, 0 or 9984); a near-constant row (0.002 + 1e-4 N(0, 1): variance ~1e-8, below eps = 1e-6).  Returns (x, kind per row)."""
    g = _gen(seed)
    x = torch.randn(rows, D, generator=g)
    kind = torch.arange(rows) % 4
    x[kind == 0] *= 1.5
    for r in (kind == 1).nonzero().flatten().tolist():
        nout = int(torch.randint(2, 5, (1,), generator=g))
        ch = torch.randperm(D, generator=g)[:nout]
        x[r, ch] = torch.sign(torch.randn(nout, generator=g)) * 10 ** (3 + torch.rand(nout, generator=g))
    consts = torch.tensor([3.0, -7.5, 0.0, 9984.0])
    for i, r in enumerate((kind == 2).nonzero().flatten().tolist()):
        x[r] = consts[i % 4]
    x[kind == 3] = 0.002 + 1e-4 * x[kind == 3]
    return x.to(torch.bfloat16).to(DEV), kind.to(DEV)


NORM_RANGE_CASES = [(600, 1280), (7, 1536), (600, 2048), (520, 3584)]


@pytest.mark.parametrize("rows,D", NORM_RANGE_CASES)
def test_layernorm_outliers_and_flat_rows(rows, D):
    x, kind = _norm_rows(rows, D, seed=500)
    w = randbf(D, seed=501)
    b = randbf(D, seed=502)
    out = torch.full_like(x, float("nan"))
    assert lib().hwocr_layernorm(p(x), p(w), p(b), p(out), rows, D, D, D, 1e-6, st()) == 0
    sync()
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    xhat = (xd - mean) * torch.rsqrt(((xd - mean) ** 2).mean(-1, keepdim=True) + 1e-6)
    want = (xhat * w.double() + b.double()).float()
    assert torch.isfinite(out.float()).all()
    # test_layernorm's bound (1 ulp + 1e-3) on every row; the ulp of the larger term |xhat w| + |b| (the output may cancel)
    mag = (xhat * w.double()).abs().float() + b.float().abs()
    assert_close_bf16(out, want, ulps=1.0, atol=1e-3, what="layernorm", mag=mag)
    # outlier rows: the ordinary channels normalise to ~1e-2 (one std is ~250), where 1e-3 would be a 10 % slack: no absolute allowance
    o = kind == 1
    assert_close_bf16(out[o], want[o], ulps=1.0, atol=0.0, what="layernorm outlier rows", mag=mag[o])


def _rms_want(x, w, gemma):
    xd = x.double()
    xhat = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6)
    return (xhat * (1.0 + w.double())).float() if gemma else w.float() * rbf(xhat.float())


@pytest.mark.parametrize("gemma", [0, 1])
@pytest.mark.parametrize("rows,D", NORM_RANGE_CASES)
def test_add_rmsnorm_outliers_flat_rows_and_a_large_residual(rows, D, gemma):
    """hwocr_add_rmsnorm with the residual write-back: h ~ the outlier / flat rows, the N(0, 1.5) ones times 1e4 (a ~1e4 residual), plus
    an update of ~1e-2 (2 fp32 slabs + bias)."""
    h, kind = _norm_rows(rows, D, seed=510)
    h[kind == 0] = (h[kind == 0].float() * 1e4).to(torch.bfloat16)
    w = randbf(D, scale=0.3, seed=511) + (0.0 if gemma else 1.0)
    bias = randbf(D, scale=1e-2, seed=512)
    slabs = randf32(2, rows, D, seed=513) * 1e-2
    h_in = h.clone()
    out = torch.full_like(h, float("nan"))
    assert lib().hwocr_add_rmsnorm(p(slabs), 2, rows * D, D, p(bias), p(h), D, p(w), p(out), D, None, rows, D, 1e-6, gemma, st()) == 0
    sync()
    y = slabs.sum(0) + bias.float()
    hin = h_in.float()
    want_h = rbf(rbf(y) + hin)
    # test_add_rmsnorm's rule for the write-back: 1 ulp, an element beyond it exactly bf16(y' + h) for a neighbour y' of bf16(y)
    assert_close_bf16_explained(h, want_h, ulps=1.0, atol=1e-3, what="residual write-back", mag=y.abs() + hin.abs(),
                                candidates=lambda idx: rbf(bf16_neighbours(rbf(y.flatten()[idx])) + hin.flatten()[idx].unsqueeze(-1)),
                                max_frac=2e-5)
    want = _rms_want(h, w, gemma)
    assert torch.isfinite(out.float()).all()
    # test_add_rmsnorm's 2.5 ulps + 1e-3; outlier rows (ordinary channels ~4e-3 after the norm) without the absolute allowance
    assert_close_bf16(out, want, ulps=2.5, atol=1e-3, what="rmsnorm")
    o = kind == 1
    assert_close_bf16(out[o], want[o], ulps=2.5, atol=0.0, what="rmsnorm outlier rows")


@pytest.mark.parametrize("gemma", [0, 1])
def test_rows16_norm_outliers_and_flat_rows(gemma):
    """The RMSNorm prologue of hwocr_gemm_rows16 (decode at <= 16 reads): write-back bit-exact, the GEMM of the normalised rows as
    test_gemm_rows16 (fp32 split-K slab, rtol 1e-4 + 6e-3)."""
    from handwritten_ocr_amd import _lib
    B, N, K, nslab = 12, 2048, 1536, 2
    w = randbf(N, K, scale=K ** -0.5, seed=521)
    wk = _tiled(w)
    h, kind = _norm_rows(B, K, seed=522)
    h[kind == 0] = (h[kind == 0].float() * 1e4).to(torch.bfloat16)            # a ~1e4 residual under a ~1e-2 update
    nw = randbf(K, scale=0.3, seed=523) + (0.0 if gemma else 1.0)
    slabs = randf32(nslab, B, K, seed=524) * 1e-2
    h_out = torch.full((B, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    blk = _lib.Rows16Norm(h_in=p(h), h_out=p(h_out), ldh=K, slabs=p(slabs), nslab=nslab, slab_stride=B * K, ld_slab=K, norm_w=p(nw),
                          eps=1e-6, gemma=gemma)
    import ctypes as C
    out = torch.full((1, B, N), float("nan"), dtype=torch.float32, device=DEV)
    assert lib().hwocr_gemm_rows16(None, 0, p(wk), p(out), N, B, N, K, 5, 1, C.byref(blk), st()) == 0
    sync()
    hp, x = _rows16_norm_ref(h, slabs, nw, gemma)
    assert torch.equal(h_out.float(), hp), "the residual update written back by the prologue"
    acc = x @ w.float().t()
    got = out.sum(0)
    assert torch.isfinite(got).all()
    assert torch.allclose(got, acc, rtol=1e-4, atol=6e-3), f"rows16 norm GEMM: {(got - acc).abs().max()}"


@pytest.mark.parametrize("rows,D", [(600, 1152), (700, 2048), (520, 3584)])
def test_norms_emitting_fp8_on_outlier_and_flat_rows(rows, D):
    """hwocr_layernorm_fp8 / hwocr_rmsnorm_fp8 = the bf16 norm, then oracle/fp8_ref.quant_rows, bit for bit.  In an outlier row the
    outliers set the row scale and the ordinary channels fall to the smallest codes: most of them subnormal."""
    x, kind = _norm_rows(rows, D, seed=530)
    w = randbf(D, scale=0.3, seed=531) + 1.0
    b = randbf(D, scale=0.2, seed=532)
    xn = torch.empty(rows, D, dtype=torch.bfloat16, device=DEV)
    for which in ("layernorm", "rms", "rms_gemma"):
        q = torch.full((rows, D), 0x7F, dtype=torch.uint8, device=DEV)
        s = torch.full((rows,), float("nan"), dtype=torch.float32, device=DEV)
        if which == "layernorm":
            assert lib().hwocr_layernorm(p(x), p(w), p(b), p(xn), rows, D, D, D, 1e-6, st()) == 0
            assert lib().hwocr_layernorm_fp8(p(x), p(w), p(b), p(q), p(s), rows, D, D, D, 1e-6, st()) == 0
        else:
            g = 1 if which == "rms_gemma" else 0
            assert lib().hwocr_add_rmsnorm(None, 0, 0, 0, None, p(x), D, p(w), p(xn), D, None, rows, D, 1e-6, g, st()) == 0
            assert lib().hwocr_rmsnorm_fp8(p(x), D, p(w), p(q), p(s), D, rows, D, 1e-6, g, st()) == 0
        sync()
        wq, ws = fp8_ref.quant_rows(xn.cpu())
        assert torch.equal(s.cpu(), ws), f"{which}: row scales"
        assert torch.equal(q.cpu(), wq.view(torch.uint8)), f"{which}: E4M3 codes"
        if which == "rms":   # the outlier rows do reach the subnormal codes (exponent field 0, nonzero)
            qo = q[kind == 1].cpu()
            assert int((((qo & 0x78) == 0) & ((qo & 0x7) != 0)).sum()) > qo.numel() // 50


# ------------------------------------------------------------------------------------------------ every E4M3 code
@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (1024, 512, 512)])
def test_gemm_wide_fp8_every_code(M, N, K, epi):
    """X and W are code matrices in which every row window of 254 holds all 254 finite codes (subnormals, +-0, +-448), with row
    scales 2^-9 .. 2^-6: the MFMA's exact products and fp32 sums against the float64 product (fp8_ref.gemm, on the device)."""
    g = _gen(600)
    xq = coverage_codes(M * K, offset=3).view(M, K).to(DEV)
    wq = coverage_codes(N * K, offset=11).view(N, K).to(DEV)
    for m in (xq, wq):
        assert set(m[0].tolist()) == set(e4m3_finite_codes().tolist())
    xs = torch.exp2(torch.empty(M).uniform_(-9, -6, generator=g)).to(DEV)
    ws = torch.exp2(torch.empty(N).uniform_(-9, -6, generator=g)).to(DEV)
    bias = randbf(N, scale=0.5, seed=601)
    res = randbf(M, N, seed=602)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    assert lib().hwocr_gemm_wide_fp8(p(xq), p(xs), p(wq), p(ws), p(bias), p(res) if epi == 1 else None, p(out), M, N, K, K, K, N, N, epi,
                                     st()) == 0
    sync()
    acc = _fp8_gemm_ref(xq, xs, wq, ws)
    _check_epilogue(out, acc, bias, res, epi, f"gemm_wide_fp8 every code epi={epi} {M}x{N}x{K}")


def _pool_rows(nrows, width, seed, exps=(-8, 8)):
    """[nrows][width] fp32: each row one value of +-448 and width - 1 values from the quantiser pool (every code and every midpoint,
    e4m3_quant_pool), walked so that the rows together hold the whole pool; row r times 2^e_r, e_r in exps (an exact scale: the
    codes are those of scale 1).  Exact in bf16."""
    g = _gen(seed)
    pool = e4m3_quant_pool()
    n = pool.numel()
    idx = (torch.arange(nrows * (width - 1)) * 7) % n                         # 7 is coprime with 506: any n consecutive hold the pool
    rows = pool[idx].view(nrows, width - 1)
    rows = torch.cat([rows, torch.where(torch.rand(nrows, 1, generator=g) < 0.5, 448.0, -448.0)], dim=1)
    rows = rows[:, torch.randperm(width, generator=g)]
    e = torch.randint(exps[0], exps[1] + 1, (nrows, 1), generator=g).float()
    return rows * torch.exp2(e)


def test_quant_rows_fp8_every_code_and_tie():
    from tests.test_ops_gpu import _quant_gpu
    x = _pool_rows(16, 512, seed=610)
    assert torch.equal(x.to(torch.bfloat16).float(), x)
    xb = x.to(torch.bfloat16).to(DEV)
    q, s = _quant_gpu(xb)
    wq, ws = fp8_ref.quant_rows(xb.cpu())
    assert torch.equal(s.cpu(), ws), "row scales"
    assert torch.equal(q.cpu(), wq.view(torch.uint8)), "E4M3 codes: a code, a rounding tie or +-448"
    assert set(q.cpu().flatten().tolist()) == set(e4m3_finite_codes().tolist())


@pytest.mark.parametrize("HD", [128, 256])
def test_kv_quant_fp8_every_code_and_tie(HD):
    """The prefill's cache fill (hwocr_kv_quant_fp8_hd; == hwocr_kv_quant_fp8 at 256) on tokens of pool values."""
    nseq, Hkv, keys, ctx = 1, 2, 64, 96
    mod = kv128 if HD == 128 else kv256
    k = _pool_rows(nseq * Hkv * keys, HD, seed=620).view(nseq, Hkv, keys, HD).to(torch.bfloat16).to(DEV)
    v = _pool_rows(nseq * Hkv * keys, HD, seed=621).view(nseq, Hkv, keys, HD).to(torch.bfloat16).to(DEV)
    vt = v.transpose(2, 3).contiguous()
    K8 = torch.full((nseq, Hkv, ctx * HD), 0xEE, dtype=torch.uint8, device=DEV)
    V8 = torch.full((nseq, Hkv, ctx * HD), 0xEE, dtype=torch.uint8, device=DEV)
    ks = torch.full((nseq, Hkv, ctx), -1.0, dtype=torch.float32, device=DEV)
    vs = torch.full((nseq, Hkv, ctx), -1.0, dtype=torch.float32, device=DEV)
    assert lib().hwocr_kv_quant_fp8_hd(p(k), p(vt), Hkv * keys * HD, keys * HD, Hkv * HD * keys, HD * keys, keys, p(K8), p(V8), p(ks),
                                       p(vs), nseq, Hkv, keys, ctx, HD, st()) == 0
    sync()
    kq, ksc = mod._quant(k)
    vq, vsc = mod._quant(v)
    assert torch.equal(ks[:, :, :keys].cpu(), ksc) and torch.equal(vs[:, :, :keys].cpu(), vsc)
    ko, vo = mod.k_offsets(ctx).view(ctx, HD)[:keys].reshape(-1), mod.v_offsets(ctx).view(HD, ctx)[:, :keys].reshape(-1)
    assert torch.equal(K8.cpu()[:, :, ko].view(nseq, Hkv, keys, HD), kq), "key codes"
    assert torch.equal(V8.cpu()[:, :, vo].view(nseq, Hkv, HD, keys), vq.transpose(2, 3)), "value codes"
    assert set(kq.flatten().tolist()) | set(vq.flatten().tolist()) == set(e4m3_finite_codes().tolist())


def _fp8kv_step(HD, Hq, Hkv, lens, ctx, nsplit, K8, V8, ks, vs, slabs, lastwg):
    """hwocr_attn_decode_qkv_fp8kv_hd at rotary position 0 for every read (rope_delta = 1 - len: cos 1, sin 0, so q / the new k are
    bf16(slab sum) as they stand).  Returns (out, K8, V8, ks, vs) after the step, on the host."""
    B = len(lens)
    G = Hq // Hkv
    W = (Hq + 2 * Hkv) * HD
    max_pos = 1024
    cos_t, sin_t = _rope_tables(max_pos, hd=HD)
    cos_d, sin_d = cos_t.to(DEV), sin_t.to(DEV)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    delta_d = torch.tensor([1 - n for n in lens], dtype=torch.int32, device=DEV)
    K8d, V8d, ksd, vsd = K8.to(DEV), V8.to(DEV), ks.to(DEV).contiguous(), vs.to(DEV).contiguous()
    po = torch.zeros(B * Hkv * nsplit * G * HD, dtype=torch.float32, device=DEV)
    pm = torch.zeros(B * Hkv * nsplit * G * 2, dtype=torch.float32, device=DEV)
    arrive = torch.zeros(B * Hkv, dtype=torch.int32, device=DEV) if lastwg else None
    out = torch.full((B, Hq * HD), float("nan"), dtype=torch.bfloat16, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib().hwocr_attn_decode_qkv_fp8kv_hd(p(slabs), slabs.shape[0], B * W, None, p(K8d), p(V8d), p(ksd), p(vsd), p(lens_d),
                                                p(delta_d), p(cos_d), p(sin_d), p(out), p(po), p(pm), p(arrive), B, Hq, Hkv, nsplit,
                                                HD ** -0.5, ctx, max_pos, HD, p(status), st()) == 0
    sync()
    assert int(status) == 0 and (arrive is None or int(arrive.abs().sum()) == 0)
    return out.cpu(), K8d.cpu(), V8d.cpu(), ksd.cpu(), vsd.cpu()


def _dequant(mod, K8, V8, ks, vs, B, Hkv, ctx, HD):
    ko, vo = mod.k_offsets(ctx), mod.v_offsets(ctx)
    kd = K8[:, :, ko].view(B, Hkv, ctx, HD).view(torch.float8_e4m3fn).float() * ks[..., None]
    vd = V8[:, :, vo].view(B, Hkv, HD, ctx).view(torch.float8_e4m3fn).float().transpose(2, 3) * vs[..., None]
    return kd, vd


def _cache_from_codes(mod, kq, vq, B, Hkv, ctx, HD):
    ko, vo = mod.k_offsets(ctx), mod.v_offsets(ctx)
    K8 = torch.zeros(B, Hkv, ctx * HD, dtype=torch.uint8)
    V8 = torch.zeros(B, Hkv, ctx * HD, dtype=torch.uint8)
    K8[:, :, ko] = kq.reshape(B, Hkv, ctx * HD)
    V8[:, :, vo] = vq.transpose(2, 3).reshape(B, Hkv, HD * ctx)
    return K8, V8


FP8KV_GEOMS = [(128, 12, 2), (256, 8, 1)]


@pytest.mark.parametrize("nsplit", [1, 4])
@pytest.mark.parametrize("HD,Hq,Hkv", FP8KV_GEOMS)
def test_decode_over_an_e4m3_cache_of_every_code(HD, Hq, Hkv, nsplit):
    """(b) The cached tokens' codes written directly: K and V hold every finite code, per-token scales 2^-9 .. 2^-6 (keys) and
    2^-2 .. 2^4 (values), zero tokens (codes 0, scale 1.0) among them, value features made of subnormal codes only.  (c) The appended token carries pool values (every code and tie,
    +-448) times 2^-12 .. 2^-4: its codes are fp8_ref's bit for bit.  The output: fp32 attention over the dequantised cache, 4 ulps of
    sum p |v| + 4e-3, as tests/test_kv_fp8_128_gpu.py."""
    mod = kv128 if HD == 128 else kv256
    ctx, lens = 320, [320, 3, 64, 200]
    B, G, W = len(lens), Hq // Hkv, (Hq + 2 * Hkv) * HD
    g = _gen(700 + HD)
    kq = coverage_codes(B * Hkv * ctx * HD, offset=1).view(B, Hkv, ctx, HD)
    vq = coverage_codes(B * Hkv * ctx * HD, offset=60).view(B, Hkv, ctx, HD)
    ks = torch.exp2(torch.empty(B, Hkv, ctx).uniform_(-9, -6, generator=g))
    vs = torch.exp2(torch.empty(B, Hkv, ctx).uniform_(-2, 4, generator=g))
    # one feature in 8 of every cached value holds positive subnormal codes only (an ordinary channel beside outliers that set the
    # scale): those outputs are made of subnormal codes alone (~0.01 x scale each), so a dequantiser that flushes them fails the bound
    sub = torch.arange(1, 8, dtype=torch.uint8)
    vq[..., 5::8] = sub[torch.randint(0, 7, vq[..., 5::8].shape, generator=g)]
    zero = torch.rand(B, Hkv, ctx, generator=g) < 0.05                      # zero tokens: what the quantiser writes for an all-zero key
    kq[zero] = 0
    ks[zero] = 1.0
    vs[torch.rand(B, Hkv, ctx, generator=g) < 0.05] = 1.0                    # values at scale 1: up to +-448
    K8, V8 = _cache_from_codes(mod, kq, vq, B, Hkv, ctx, HD)
    # the appended token (slot len - 1): pool rows; q ~ N(0, 1)
    y = torch.randn(B, W, generator=g)
    nk = _pool_rows(B * Hkv, HD, seed=710, exps=(-12, -8)).view(B, Hkv * HD)     # |k| <= 1.75: logits of the old keys' spread
    nv = _pool_rows(B * Hkv, HD, seed=711, exps=(-8, -4)).view(B, Hkv * HD)
    y[:, Hq * HD:(Hq + Hkv) * HD], y[:, (Hq + Hkv) * HD:] = nk, nv
    y = rbf(y)
    slabs = y.unsqueeze(0).to(DEV).contiguous()
    old = torch.zeros(B, Hkv, ctx, dtype=torch.bool)
    for b, n in enumerate(lens):
        old[b, :, : n - 1] = True
    assert set(kq[old].flatten().tolist()) | set(vq[old].flatten().tolist()) == set(e4m3_finite_codes().tolist())
    outs = []
    for lastwg in ([False, True] if nsplit > 1 else [False]):
        out, K8o, V8o, kso, vso = _fp8kv_step(HD, Hq, Hkv, lens, ctx, nsplit, K8, V8, ks, vs, slabs, lastwg)
        outs.append(out)
        # (c) the appended token: fp8_ref of the planted values, bit for bit; nothing else moved
        # the step sums its slabs from +0: a planted -0 arrives as +0 (as in the bf16-cache step), so the reference quantises nk + 0
        nkq, nks = mod._quant((nk + 0.0).view(B, Hkv, HD).to(torch.bfloat16))
        nvq, nvs = mod._quant((nv + 0.0).view(B, Hkv, HD).to(torch.bfloat16))
        K8w, V8w, ksw, vsw = K8.clone(), V8.clone(), ks.clone(), vs.clone()
        ko2, vo2 = mod.k_offsets(ctx).view(ctx, HD), mod.v_offsets(ctx).view(HD, ctx)
        for b, n in enumerate(lens):
            K8w[b][:, ko2[n - 1]] = nkq[b]
            V8w[b][:, vo2[:, n - 1]] = nvq[b]
            ksw[b, :, n - 1], vsw[b, :, n - 1] = nks[b], nvs[b]
        assert torch.equal(K8o, K8w) and torch.equal(V8o, V8w), "cache codes: the appended token's, or another slot moved"
        assert torch.equal(kso, ksw) and torch.equal(vso, vsw), "cache scales"
        # (b) the attention over the dequantised cache
        kd, vd = _dequant(mod, K8o, V8o, kso, vso, B, Hkv, ctx, HD)
        for b, n in enumerate(lens):
            q = y[b, : Hq * HD].view(Hq, 1, HD)
            want = _sdpa_ref(q.double(), kd[b, :, :n].double(), vd[b, :, :n].double(), False, HD ** -0.5).reshape(Hq * HD).float()
            mag = _sdpa_ref(q.double(), kd[b, :, :n].double(), vd[b, :, :n].abs().double(), False, HD ** -0.5).reshape(Hq * HD).float()
            assert_close_bf16(out[b], want, ulps=4.0, atol=4e-3, what=f"every-code e4m3 attention hd {HD}, read {b} len {n}", mag=mag)
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), "last-workgroup merge differs from the merge launch"
    # every finite code reached the appended token's quantiser (-0 too: the tie -2^-10 rounds to it)
    assert set(nkq.flatten().tolist()) | set(nvq.flatten().tolist()) == set(e4m3_finite_codes().tolist())


# ------------------------------------------------------------------------------------------------ E4M3 cache against bf16 attention
def _outlier_keys(B, Hkv, ctx, HD, g):
    """bf16 keys N(0, 1) with three RoPE-rotated outlier channel pairs (d, d + HD/2) of amplitude 20 (ASSUMED, not measured): the pair
    turns with the token position at the pair's rotary frequency, as a post-RoPE key of a real checkpoint would."""
    k = torch.randn(B, Hkv, ctx, HD, generator=g)
    inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=torch.float64) / HD))
    pos = torch.arange(ctx, dtype=torch.float64)
    for d in (3, 21, 47):
        th = pos * inv[d] + float(torch.rand(1, generator=g)) * 6.28
        amp = 20.0 * (1 + 0.1 * torch.randn(B, Hkv, 1, generator=g))
        k[..., d] = (amp * torch.cos(th)).float()
        k[..., d + HD // 2] = (amp * torch.sin(th)).float()
    return k.to(torch.bfloat16)


WORST = {}


@pytest.mark.parametrize("nsplit", [1, 4])
@pytest.mark.parametrize("HD,Hq,Hkv", FP8KV_GEOMS)
def test_e4m3_cache_against_bf16_attention_within_the_bound(HD, Hq, Hkv, nsplit):
    """The E4M3 cache's output against the float64 attention over the UNQUANTISED bf16 keys / values: within
    (e^{2 eps} - 1) sum p_j |v_j| + max_j |v_j - deq(v_j)| (tests/_ranges.kv8_error_bound, eps = scale max_j |q.(k_j - deq(k_j))|,
    from the actual codes), plus the kernel's own 4 ulps + 4e-3 over the codes (test_decode_over_an_e4m3_cache_of_every_code)."""
    mod = kv128 if HD == 128 else kv256
    ctx, lens = 320, [320, 100, 257]
    B, G, W = len(lens), Hq // Hkv, (Hq + 2 * Hkv) * HD
    scale = HD ** -0.5
    g = _gen(800 + HD)
    k = _outlier_keys(B, Hkv, ctx, HD, g)
    v = torch.randn(B, Hkv, ctx, HD, generator=g).to(torch.bfloat16)
    kq, ksc = mod._quant(k)
    vq, vsc = mod._quant(v)
    K8, V8 = _cache_from_codes(mod, kq, vq, B, Hkv, ctx, HD)
    y = torch.randn(B, W, generator=g)
    y[:, Hq * HD:(Hq + Hkv) * HD] = _outlier_keys(B, Hkv, 1, HD, g).float().reshape(B, Hkv * HD)   # the appended key: outliers too
    y = rbf(y)
    slabs = y.unsqueeze(0).to(DEV).contiguous()
    out, K8o, V8o, kso, vso = _fp8kv_step(HD, Hq, Hkv, lens, ctx, nsplit, K8, V8, ksc, vsc, slabs, lastwg=nsplit > 1)
    kd, vd = _dequant(mod, K8o, V8o, kso, vso, B, Hkv, ctx, HD)
    kb, vb = k.float().clone(), v.float().clone()
    for b, n in enumerate(lens):      # the bf16 key / value the step appended (position 0: bf16(slab) as it stands)
        kb[b, :, n - 1] = y[b, Hq * HD:(Hq + Hkv) * HD].view(Hkv, HD)
        vb[b, :, n - 1] = y[b, (Hq + Hkv) * HD:].view(Hkv, HD)
    worst_bound, worst_total = 0.0, 0.0
    for b, n in enumerate(lens):
        for h in range(Hkv):
            q = y[b, h * G * HD:(h + 1) * G * HD].view(G, HD).double()
            o_bf16 = torch.softmax(scale * q @ kb[b, h, :n].double().t(), -1) @ vb[b, h, :n].double()
            bound = kv8_error_bound(q, kb[b, h, :n], kd[b, h, :n], vb[b, h, :n], vd[b, h, :n], scale)
            pq = torch.softmax(scale * q @ kd[b, h, :n].double().t(), -1)
            mag = torch.maximum(pq @ vd[b, h, :n].double().abs(), o_bf16.abs())
            own = 4.0 * torch.exp2(torch.floor(torch.log2(mag.clamp_min(1e-30))) - 7.0) + 4e-3
            got = out[b].view(Hq, HD)[h * G:(h + 1) * G].double()
            err = (got - o_bf16).abs()
            assert bool((err <= bound + own).all()), (f"read {b} kv head {h}: E4M3 output off the bf16 attention by "
                                                     f"{float((err - bound - own).max()):.4g} beyond the bound")
            worst_bound = max(worst_bound, float((err / bound).max()))
            worst_total = max(worst_total, float((err / (bound + own)).max()))
    WORST[(HD, nsplit)] = (worst_bound, worst_total)
    print(f"\nE4M3 cache vs bf16 attention, hd {HD} nsplit {nsplit}: worst |err| / bound {worst_bound:.3f}, "
          f"worst |err| / (bound + kernel allowance) {worst_total:.3f}")
