"""The E4M3 KV cache of 128-wide heads (Qwen2-VL / Qwen2.5-VL) on the MI355X, operator level, through the C ABI.  Same contract as the
256-wide cache (tests/test_kv_fp8_gpu.py): the quantiser bit for bit against oracle/fp8_ref.py, the layout against its Python
restatement, the attention against the fp32 product of the SAME codes and scales (HF has no fp8 path).
  * hwocr_kv_quant_fp8_hd            the prefill's cache fill at head_dim 128
  * hwocr_attn_decode_qkv_fp8kv_hd   the fused decode step: both geometries (8 waves at nsplit 1, 4 waves x nsplit + merge)
  * hwocr_prefill over an E4M3 cache leaves the quantisation of what a bf16-cache prefill writes"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._gpu_util import DEV, assert_close_bf16, lib, p, randbf, randf32, rbf, st  # noqa: E402
from tests.test_ops_gpu import _rope_tables, _sdpa_ref  # noqa: E402

HD = 128


def k_offsets(ctx):
    """byte offset of code (key, d) inside a (read, kv head) region: csrc/common.h kv8_k<128> restated."""
    key = torch.arange(ctx).view(-1, 1)
    d = torch.arange(HD).view(1, -1)
    kl = key & 31
    t = (kl >> 2) & 1
    c = ((kl >> 3) << 2) | (kl & 3)
    s, qd = d >> 5, (d >> 3) & 3
    return (((((key >> 5) * 2 + t) * (HD // 64) + (s >> 1)) * 64 + qd * 16 + c) * 16 + (s & 1) * 8 + (d & 7)).reshape(-1)


def v_offsets(ctx):
    """... of code (d, key): kv8_v<128>."""
    d = torch.arange(HD).view(-1, 1)
    key = torch.arange(ctx).view(1, -1)
    kl = key & 31
    return ((((key >> 5) * (HD // 32) + (d >> 5)) * 64 + (kl >> 3) * 16 + (d & 15)) * 16 + ((d >> 4) & 1) * 8 + (kl & 7)).reshape(-1)


def test_layout_maps_are_permutations():
    for ctx in (32, 96, 320, 512):
        for off in (k_offsets(ctx), v_offsets(ctx)):
            assert sorted(off.tolist()) == list(range(ctx * HD))


def test_a_lanes_16_bytes_are_one_fragment_and_a_block_is_contiguous():
    """Every 16-byte group holds the 8 + 8 codes of ONE lane's fragments (K: one key, 16 features of two k-steps; V^T: the same 8
    keys of feature rows d and d + 16, two d-tiles), and a 32-key block is one contiguous 4-KiB run of each map."""
    ctx = 64
    ko, vo = k_offsets(ctx).view(ctx, HD), v_offsets(ctx).view(HD, ctx)
    for key in range(ctx):
        assert set((ko[key] >> 4).tolist()) <= set(range((key >> 5) * 256, (key >> 5) * 256 + 256))
    grp = {}
    for key in range(ctx):
        for d in range(HD):
            grp.setdefault(int(ko[key, d]) >> 4, set()).add(key)
    assert all(len(v) == 1 for v in grp.values())
    for key in range(ctx):
        assert set((vo[:, key] >> 4).tolist()) <= set(range((key >> 5) * 256, (key >> 5) * 256 + 256))
    grp = {}
    for d in range(HD):
        for key in range(ctx):
            grp.setdefault(int(vo[d, key]) >> 4, set()).add((d, key >> 3))
    for v in grp.values():
        rows, octets = {r for r, _ in v}, {o for _, o in v}
        assert len(octets) == 1 and len(rows) == 2 and max(rows) - min(rows) == 16 and min(rows) % 32 < 16


def _quant(x):
    """oracle quantiser on rows of x [..., 128] -> (codes uint8, scales fp32)."""
    from oracle import fp8_ref

    q, s = fp8_ref.quant_rows(x.reshape(-1, x.shape[-1]).cpu())
    return q.view(torch.uint8).reshape(x.shape), s.reshape(x.shape[:-1])


@pytest.mark.parametrize("nseq,Hkv,keys,ctx", [(3, 2, 64, 128), (2, 4, 4160, 4224), (1, 2, 96, 320)])
def test_kv_quant_fp8_hd128_codes_scales_and_layout(nseq, Hkv, keys, ctx):
    k = randbf(nseq, Hkv, keys, HD, seed=51)
    v = randbf(nseq, Hkv, keys, HD, scale=3.0, seed=52)
    k[0, 0, 5] = 0                                                     # an all-zero token: scale 1, codes 0
    v[0, -1, 7] = 0
    vt = v.transpose(2, 3).contiguous()
    K8 = torch.full((nseq, Hkv, ctx * HD), 0xEE, dtype=torch.uint8, device=DEV)
    V8 = torch.full((nseq, Hkv, ctx * HD), 0xEE, dtype=torch.uint8, device=DEV)
    ks = torch.full((nseq, Hkv, ctx), -1.0, dtype=torch.float32, device=DEV)
    vs = torch.full((nseq, Hkv, ctx), -1.0, dtype=torch.float32, device=DEV)
    assert lib().hwocr_kv_quant_fp8_hd(p(k), p(vt), Hkv * keys * HD, keys * HD, Hkv * HD * keys, HD * keys, keys, p(K8), p(V8), p(ks),
                                       p(vs), nseq, Hkv, keys, ctx, HD, st()) == 0
    torch.cuda.synchronize()
    kq, ksc = _quant(k)
    vq, vsc = _quant(v)
    assert torch.equal(ks[:, :, :keys].cpu(), ksc) and torch.equal(vs[:, :, :keys].cpu(), vsc)
    assert bool((ks[:, :, keys:] == -1).all()) and bool((vs[:, :, keys:] == -1).all())
    assert float(ks[0, 0, 5]) == 1.0 and float(vs[0, -1, 7]) == 1.0
    ko, vo = k_offsets(ctx).view(ctx, HD)[:keys].reshape(-1), v_offsets(ctx).view(HD, ctx)[:, :keys].reshape(-1)
    assert torch.equal(K8.cpu()[:, :, ko].view(nseq, Hkv, keys, HD), kq)
    assert torch.equal(V8.cpu()[:, :, vo].view(nseq, Hkv, HD, keys), vq.transpose(2, 3))
    for buf, off in ((K8, ko), (V8, vo)):   # nothing past `keys` is written
        untouched = torch.ones(ctx * HD, dtype=torch.bool)
        untouched[off] = False
        assert bool((buf.cpu()[:, :, untouched] == 0xEE).all())


def _lens(B, ctx, g):
    lens = torch.randint(2, ctx, (B,), generator=g).tolist()
    special = [1, ctx, 33, 64]   # new slot opens a block / last cache position / second block / last of a block
    lens[: min(B, 4)] = special[: min(B, 4)]
    return lens


# (Hq, Hkv): the Qwen2-VL-2B (G = 6) and Qwen2.5-VL-7B (G = 7) head shapes; B: one read, few, the rows16 edge, past it, the bench's 252
@pytest.mark.parametrize("Hq,Hkv", [(12, 2), (28, 4)])
@pytest.mark.parametrize("B", [1, 3, 16, 17, 252])
@pytest.mark.parametrize("nsplit", [1, 3, 16])
def test_attn_decode_qkv_over_the_e4m3_cache_hd128(Hq, Hkv, B, nsplit):
    """(1) The appended token: exactly the oracle quantisation of the bf16 key / value the bf16-cache kernel appends, nothing else of
    the cache moves.  (2) The output: the fp32 attention over the dequantised cache, 4 bf16 ulps.  (3) With splits: last-workgroup
    merge and merge launch give identical bytes."""
    ctx, nslab, max_pos = 320, 2, 1024
    W = (Hq + 2 * Hkv) * HD
    G = Hq // Hkv
    g = torch.Generator().manual_seed(13 + B + nsplit)
    lens = _lens(B, ctx, g)
    delta = torch.randint(-1, 300, (B,), generator=g).tolist()
    delta[0] = 0
    slabs = randf32(nslab, B, W, seed=911)
    cos_t, sin_t = _rope_tables(max_pos, hd=HD)
    cos_d, sin_d = cos_t.to(DEV), sin_t.to(DEV)
    k = randbf(B, Hkv, ctx, HD, seed=26)
    v = randbf(B, Hkv, ctx, HD, scale=2.0, seed=27)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    delta_d = torch.tensor(delta, dtype=torch.int32, device=DEV)
    # what the bf16-cache kernel (row layout) appends: the reference for the new token's k / v
    Kb, Vb = k.clone(), v.transpose(2, 3).contiguous()
    outb = torch.zeros(B, Hq * HD, dtype=torch.bfloat16, device=DEV)
    stb = torch.zeros(1, dtype=torch.int32, device=DEV)
    po = torch.zeros(B * Hkv * nsplit * G * HD, dtype=torch.float32, device=DEV)
    pm = torch.zeros(B * Hkv * nsplit * G * 2, dtype=torch.float32, device=DEV)
    assert lib().hwocr_attn_decode_qkv(p(slabs), nslab, B * W, None, p(Kb), p(Vb), p(lens_d), p(delta_d), p(cos_d), p(sin_d), p(outb), p(po),
                                       p(pm), None, B, Hq, Hkv, nsplit, Hkv * ctx * HD, ctx * HD, Hkv * HD * ctx, HD * ctx, ctx, HD ** -0.5,
                                       HD, 0, ctx, max_pos, p(stb), st()) == 0
    torch.cuda.synchronize()
    assert int(stb) == 0
    slot = torch.tensor(lens) - 1
    ar = torch.arange(B)
    Kbc, Vbc = Kb.cpu(), Vb.cpu()
    new_k = Kbc[ar, :, slot]                      # [B, Hkv, 128]
    new_v = Vbc[ar, :, :, slot]
    nkq, nks = _quant(new_k)
    nvq, nvs = _quant(new_v)
    # the E4M3 cache of the OLD tokens, built with the oracle quantiser and the Python layout maps
    kq, ksc = _quant(k)
    vq, vsc = _quant(v)
    ko, vo = k_offsets(ctx), v_offsets(ctx)
    ko2, vo2 = ko.view(ctx, HD), vo.view(HD, ctx)
    K8 = torch.zeros(B, Hkv, ctx * HD, dtype=torch.uint8)
    V8 = torch.zeros(B, Hkv, ctx * HD, dtype=torch.uint8)
    K8[:, :, ko] = kq.reshape(B, Hkv, ctx * HD)
    V8[:, :, vo] = vq.transpose(2, 3).reshape(B, Hkv, HD * ctx)
    # the expected cache after the step: the old one with the new token's codes / scales at its slot
    K8w, V8w, ksw, vsw = K8.clone(), V8.clone(), ksc.clone(), vsc.clone()
    for b in range(B):
        K8w[b][:, ko2[slot[b]]] = nkq[b]
        V8w[b][:, vo2[:, slot[b]]] = nvq[b]
        ksw[b, :, slot[b]] = nks[b]
        vsw[b, :, slot[b]] = nvs[b]
    y = rbf(slabs.sum(0).cpu())                                                       # [B, W]
    check = sorted({0, 1, 2, 3, B // 2, B - 1} & set(range(B)))
    outs = []
    for lastwg in ([False, True] if nsplit > 1 else [False]):
        K8d, V8d, ksd, vsd = K8.to(DEV), V8.to(DEV), ksc.to(DEV).contiguous(), vsc.to(DEV).contiguous()
        arrive = torch.zeros(B * Hkv, dtype=torch.int32, device=DEV) if lastwg else None
        out = torch.zeros(B, Hq * HD, dtype=torch.bfloat16, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        po.zero_()
        pm.zero_()
        assert lib().hwocr_attn_decode_qkv_fp8kv_hd(p(slabs), nslab, B * W, None, p(K8d), p(V8d), p(ksd), p(vsd), p(lens_d), p(delta_d),
                                                    p(cos_d), p(sin_d), p(out), p(po), p(pm), p(arrive), B, Hq, Hkv, nsplit, HD ** -0.5, ctx,
                                                    max_pos, HD, p(status), st()) == 0
        torch.cuda.synchronize()
        assert int(status) == 0 and (arrive is None or int(arrive.abs().sum()) == 0)
        outs.append(out.cpu())
        # (1) the appended token, and nothing else of the cache moved
        Kc, Vc, ksc_, vsc_ = K8d.cpu(), V8d.cpu(), ksd.cpu(), vsd.cpu()
        assert torch.equal(Kc, K8w), "key codes: the appended token's, or another slot moved"
        assert torch.equal(Vc, V8w), "value codes: the appended token's, or another slot moved"
        assert torch.equal(ksc_, ksw) and torch.equal(vsc_, vsw), "scales"
        # (2) the attention over the dequantised cache
        kd = Kc[:, :, ko].view(B, Hkv, ctx, HD).view(torch.float8_e4m3fn).float() * ksc_[..., None]
        vd = Vc[:, :, vo].view(B, Hkv, HD, ctx).view(torch.float8_e4m3fn).float().transpose(2, 3) * vsc_[..., None]
        for b in check:
            n, pos = lens[b], lens[b] - 1 + delta[b]
            q = y[b, : Hq * HD].view(Hq, HD)
            cs, sn = cos_t[pos].float(), sin_t[pos].float()
            x1, x2 = q[:, : HD // 2], q[:, HD // 2:]
            qr = torch.cat([rbf(rbf(x1 * cs) + rbf(-x2 * sn)), rbf(rbf(x2 * cs) + rbf(x1 * sn))], dim=1)
            want = _sdpa_ref(qr.view(Hq, 1, HD), kd[b, :, :n], vd[b, :, :n], False, HD ** -0.5).reshape(Hq * HD)
            # the softmax weights enter the PV product as bf16 (weight x value scale, rounded): an output that cancels carries the
            # rounding of its terms, so the ulp is taken of sum_i p_i |v_i| (the same bf16 P as the bf16-cache kernel's)
            mag = _sdpa_ref(qr.view(Hq, 1, HD), kd[b, :, :n], vd[b, :, :n].abs(), False, HD ** -0.5).reshape(Hq * HD)
            assert_close_bf16(outs[-1][b], want, ulps=4.0, atol=4e-3, what=f"e4m3-cache attention, read {b} len {n}", mag=mag)
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), "last-workgroup merge differs from the merge launch"


def test_decode_qkv_fp8kv_hd_refuses_what_it_does_not_cover():
    """head_dim other than 128 / 256, and a ctx that is not a multiple of 32, are rejected before anything is launched."""
    one = torch.zeros(64, dtype=torch.float32, device=DEV)
    args = lambda hd, ctx: (p(one), 1, 64, None, p(one), p(one), p(one), p(one), p(one), p(one), p(one), p(one), p(one), p(one), p(one),
                            None, 1, 2, 1, 1, 1.0, ctx, 64, hd, None, st())
    assert lib().hwocr_attn_decode_qkv_fp8kv_hd(*args(64, 64)) == 1
    assert lib().hwocr_attn_decode_qkv_fp8kv_hd(*args(128, 48)) == 1
    assert lib().hwocr_kv_quant_fp8_hd(p(one), p(one), 0, 0, 0, 0, 64, p(one), p(one), p(one), p(one), 1, 1, 32, 64, 64, st()) == 1


def _untile_k(buf, ctx):
    """bf16 fragment-tiled K region [ctx * 128] (csrc/common.h kv_tiled_k) -> rows [ctx][128]."""
    key = torch.arange(ctx).view(-1, 1)
    d = torch.arange(HD).view(1, -1)
    kl = key & 31
    t = (kl >> 2) & 1
    c = ((kl >> 3) << 2) | (kl & 3)
    off = (((((key >> 5) * 2 + t) * 4 + (d >> 5)) * 64 + ((d >> 3) & 3) * 16 + c) << 3) + (d & 7)
    return buf[..., off.reshape(-1)].reshape(*buf.shape[:-1], ctx, HD)


def _untile_v(buf, ctx):
    """... V^T region (kv_tiled_v) -> rows [128][ctx]."""
    d = torch.arange(HD).view(-1, 1)
    key = torch.arange(ctx).view(1, -1)
    kl = key & 31
    off = ((((key >> 5) * 8 + (d >> 4)) * 64 + (kl >> 3) * 16 + (d & 15)) << 3) + (kl & 7)
    return buf[..., off.reshape(-1)].reshape(*buf.shape[:-1], HD, ctx)


@pytest.mark.parametrize("family,name", [("qwen2_vl", "tiny"), ("qwen2_5_vl", "tiny25")])
def test_prefill_fills_the_e4m3_cache_with_the_quantised_bf16_prompt(family, name):
    """hwocr_prefill over an E4M3 cache (one prefill chunk per read pair: prefill_batch 2) leaves, for every prompt position, exactly
    oracle quant_rows of the bf16 K / V^T a bf16-cache prefill of the same prompts writes."""
    from PIL import Image

    from handwritten_ocr_amd import engine, imageproc
    from tests import _golden

    cfg = engine.preset(name)
    g = _golden.tiny_case("bf16", family)
    pages = [imageproc.prepare_page(Image.fromarray(g[f"{c}.page"].numpy(), "RGB"), cfg.patch_size, cfg.merge, cfg.min_pixels,
                                    cfg.max_pixels) for c in ("a", "b", "a")]
    prompts = [g[f"{c}.input_ids"].numpy() for c in ("a", "b", "a")]
    sd = _golden.tiny_weights(torch.bfloat16, family)
    ctx, R = 256, 4
    e16 = engine.ReadEngine(cfg, sd, max_reads=R, ctx=ctx, vit_batch=2, prefill_batch=2, fp8_kv=False)
    e8 = engine.ReadEngine(cfg, sd, max_reads=R, ctx=ctx, vit_batch=2, prefill_batch=2, fp8_kv=True)
    try:
        e16.generate(pages, prompts, max_new=1)
        e8.generate(pages, prompts, max_new=1)
        torch.cuda.synchronize()
        L, Hkv, n = cfg.layers, cfg.kv_heads, len(pages)
        Tmin = min(len(q) for q in prompts)
        kb = _untile_k(e16.k_cache.cpu().view(L, R, Hkv, ctx * HD), ctx)[:, :n, :, :Tmin]          # [L, n, Hkv, T, 128]
        vb = _untile_v(e16.vt_cache.cpu().view(L, R, Hkv, ctx * HD), ctx)[:, :n, :, :, :Tmin]      # [L, n, Hkv, 128, T]
        kq, ks = _quant(kb.contiguous())
        vq, vs = _quant(vb.transpose(3, 4).contiguous())
        K8 = e8.k_cache.cpu().view(L, R, Hkv, ctx * HD)[:, :n]
        V8 = e8.vt_cache.cpu().view(L, R, Hkv, ctx * HD)[:, :n]
        ko, vo = k_offsets(ctx).view(ctx, HD)[:Tmin].reshape(-1), v_offsets(ctx).view(HD, ctx)[:, :Tmin].reshape(-1)
        assert torch.equal(K8[..., ko].view(L, n, Hkv, Tmin, HD), kq)
        assert torch.equal(V8[..., vo].view(L, n, Hkv, HD, Tmin), vq.transpose(3, 4))
        assert torch.equal(e8.k_scale.cpu().view(L, R, Hkv, ctx)[:, :n, :, :Tmin], ks)
        assert torch.equal(e8.v_scale.cpu().view(L, R, Hkv, ctx)[:, :n, :, :Tmin], vs)
        assert int(np.count_nonzero(kq.numpy())) > 0
    finally:
        e16.close()
        e8.close()
