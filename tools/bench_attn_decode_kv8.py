"""Time the fused decode attention of 128-wide heads over the bf16 fragment-tiled cache and over the E4M3 cache, alone, at a bench
geometry: 252 reads, one workgroup per (read, kv head) (nsplit 1), every read at the bench's mean context (prompt 1328 + 256 generated).
Cold cache: NCOPY layer-sized caches are walked in turn, as the 28 layers of a decode step are (the E4M3 cache of one layer, ~210 MB at
the 2B shape, would otherwise sit in the 256 MB Infinity Cache).  Also the workload for a rocprofv3 --pmc pass.  Run on the GPU box.
usage: bench_attn_decode_kv8.py [2b|7b] [iters]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from handwritten_ocr_amd import _lib  # noqa: E402

shape = sys.argv[1] if len(sys.argv) > 1 else "2b"
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 40
Hq, Hkv = (12, 2) if shape == "2b" else (28, 4)
B, HD, ctx, L, NCOPY, max_pos = 252, 128, 2048, 1584, 4, 4096
dev = "cuda"
lib, p = _lib.hip(), _lib.ptr
W = (Hq + 2 * Hkv) * HD
g = torch.Generator(device="cpu").manual_seed(0)
slabs = torch.randn(1, B, W, generator=g).to(dev)
lens = torch.full((B,), L, dtype=torch.int32, device=dev)
delta = torch.zeros(B, dtype=torch.int32, device=dev)
ang = torch.arange(max_pos, dtype=torch.float).unsqueeze(-1) * (1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=torch.float) / HD)))
cos_t, sin_t = ang.cos().to(torch.bfloat16).to(dev), ang.sin().to(torch.bfloat16).to(dev)
out = torch.zeros(B, Hq * HD, dtype=torch.bfloat16, device=dev)
status = torch.zeros(1, dtype=torch.int32, device=dev)
n = B * Hkv * ctx * HD
kb = [torch.randn(n, generator=g).to(torch.bfloat16).to(dev) for _ in range(2 * NCOPY)]
k8 = [torch.randint(0, 0x70, (n,), generator=g, dtype=torch.uint8).to(dev) for _ in range(2 * NCOPY)]   # (no NaN codes)
sc = [torch.full((B * Hkv * ctx,), 0.01, dtype=torch.float32, device=dev) for _ in range(2 * NCOPY)]
st = _lib.stream_handle()


def bf16(i):
    K, V = kb[2 * i], kb[2 * i + 1]
    return lib.hwocr_attn_decode_qkv(p(slabs), 1, B * W, None, p(K), p(V), p(lens), p(delta), p(cos_t), p(sin_t), p(out), None, None, None,
                                     B, Hq, Hkv, 1, Hkv * ctx * HD, ctx * HD, Hkv * ctx * HD, ctx * HD, ctx, HD ** -0.5, HD, 1, ctx, max_pos,
                                     p(status), st)


def e4m3(i):
    K, V, ks, vs = k8[2 * i], k8[2 * i + 1], sc[2 * i], sc[2 * i + 1]
    return lib.hwocr_attn_decode_qkv_fp8kv_hd(p(slabs), 1, B * W, None, p(K), p(V), p(ks), p(vs), p(lens), p(delta), p(cos_t), p(sin_t),
                                              p(out), None, None, None, B, Hq, Hkv, 1, HD ** -0.5, ctx, max_pos, HD, p(status), st)


for name, fn, kv_bytes in (("bf16", bf16, 2 * B * Hkv * L * HD * 2), ("e4m3", e4m3, 2 * B * Hkv * L * (HD + 4))):
    for i in range(NCOPY):
        assert fn(i) == 0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for it in range(iters):
        assert fn(it % NCOPY) == 0
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    print(f"{shape} {name}: {us:.1f} us per launch, K + V^T {kv_bytes / 1e6:.0f} MB -> {kv_bytes / us / 1e6:.2f} TB/s")
    assert int(status) == 0
