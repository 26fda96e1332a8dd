"""The E4M3 KV cache of 128-wide heads through the engine (ReadEngine fp8_kv / HWOCR_KV_DTYPE=e4m3) on the MI355X.

HF has no fp8 path, so the effect of the cache on the OUTPUT is a stated tolerance of this repo, not a pinned parity: the trained tiny
Qwen2-VL / Qwen2.5-VL checkpoints (tests/golden/trained_*) read free-running with an E4M3 cache must stay within the accuracy bar of
tests/test_trained_gpu.py (mean CER <= 0.005 against HF's bf16 text) on one lane, with graph replay, on two lanes and through the
drop-in.  The printed lines say how many token streams differ from HF's."""
import os

import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from tests._golden import mean_cer, tiny_weights, trained_dir, trained_meta, trained_page  # noqa: E402

CER_BAR = 0.005
QWEN = (("qwen2_vl", "tiny"), ("qwen2_5_vl", "tiny25"))


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("family,name", QWEN)
def test_fp8_kv_true_gives_an_e4m3_cache_at_head_dim_128(family, name, fp8, monkeypatch):
    from handwritten_ocr_amd import engine

    monkeypatch.delenv("HWOCR_KV_DTYPE", raising=False)
    cfg = engine.preset(name)
    assert cfg.head_dim == 128
    e = engine.ReadEngine(cfg, tiny_weights(torch.bfloat16, family), max_reads=4, ctx=256, vit_batch=2, prefill_batch=2, fp8=fp8,
                          fp8_kv=True)
    try:
        assert e.fp8_kv and e.k_cache.dtype == torch.uint8 and e.vt_cache.dtype == torch.uint8
        assert e.kv.fp8 == 1 and e.kv.tiled == 0 and e.kv.k_scale and e.kv.v_scale
        assert e.k_cache.numel() == cfg.layers * 4 * cfg.kv_heads * e.ctx * 128          # one byte per cached element
        assert e.k_scale.numel() == cfg.layers * 4 * cfg.kv_heads * e.ctx                # one scale per token and kv head
        ln = e.lane()
        try:
            assert ln.fp8_kv and ln.k_cache.dtype == torch.uint8 and ln.k_cache.data_ptr() != e.k_cache.data_ptr()
            assert ln.k_scale.data_ptr() != e.k_scale.data_ptr()
        finally:
            ln.close()
    finally:
        e.close()


@pytest.mark.parametrize("family,name", QWEN)
def test_the_default_cache_of_a_qwen_engine_is_still_bf16_tiled(family, name, monkeypatch):
    from handwritten_ocr_amd import engine

    monkeypatch.delenv("HWOCR_KV_DTYPE", raising=False)
    monkeypatch.delenv("HWOCR_FP8_KV", raising=False)
    for fp8 in (False, True):
        e = engine.ReadEngine(engine.preset(name), tiny_weights(torch.bfloat16, family), max_reads=2, ctx=256, vit_batch=2,
                              prefill_batch=2, fp8=fp8)
        try:
            assert not e.fp8_kv and e.k_cache.dtype == torch.bfloat16 and e.kv.tiled == 1 and e.kv.fp8 == 0
        finally:
            e.close()


class _Trained:
    def __init__(self, family, **kw):
        from handwritten_ocr_amd import engine, tokenizer
        from handwritten_ocr_amd.compat import config

        self.family = family
        self.meta = trained_meta(family)
        self.dir = trained_dir(family)
        cfg, sd = engine.load_checkpoint_dir(self.dir, device="cuda")
        cfg.min_pixels, cfg.max_pixels = config.OCR_MIN_PIXELS, config.OCR_MAX_PIXELS
        self.cfg = cfg
        self.eng = engine.ReadEngine(cfg, sd, max_reads=64, ctx=512, vit_batch=12, prefill_batch=16, fp8_kv=True, **kw)
        assert self.eng.fp8_kv and self.eng.k_cache.dtype == torch.uint8
        self.proc = tokenizer.Processor(cfg, tokenizer.HFTokenizer(cfg, self.dir), template_dir=self.dir)
        self.cases = self.meta["cases"]
        prepared = [self.proc.prepare(Image.fromarray(trained_page(c), "RGB"), self.meta["prompt"]) for c in self.cases]
        self.pages = [p for p, _ in prepared]
        self.prompts = [q for _, q in prepared]
        self.hf_texts = [c["hf_text"] for c in self.cases]
        self.n = self.meta["max_new_tokens"]

    def reads(self, count):
        idx = [i % len(self.cases) for i in range(count)]
        return idx, [self.pages[i] for i in idx], [self.prompts[i] for i in idx]

    def check(self, idx, streams, what):
        texts = [self.proc.decode(t, skip_special_tokens=True) for t in streams]
        m = mean_cer([self.hf_texts[i] for i in idx], texts)
        differing = sum(t != self.cases[i]["hf_tokens"] for i, t in zip(idx, streams))
        print(f"[e4m3 cache, trained {self.family}] {what}: mean CER {m:.4f} vs HF's bf16 text, {differing}/{len(idx)} token streams differ")
        assert m <= CER_BAR, f"{self.family} {what}: mean CER {m:.4f} vs HF's bf16 text ({differing} token streams differ)"
        return m, differing


@pytest.fixture(scope="module", params=("qwen2_vl", "qwen2_5_vl"))
def trained(request):
    t = _Trained(request.param)
    yield t
    t.eng.close()


@pytest.mark.parametrize("reads", [8, 24, 64])
def test_e4m3_cache_free_running_within_the_cer_bar(trained, reads):
    """One lane; the second call replays the decode graph captured by the first (same bytes)."""
    idx, pages, prompts = trained.reads(reads)
    first = trained.eng.generate(pages, prompts, max_new=trained.n)
    trained.check(idx, first, f"{reads} reads in flight")
    again = trained.eng.generate(pages, prompts, max_new=trained.n)
    assert again == first, "graph replay over the E4M3 cache differs from the captured run"


def test_e4m3_cache_on_two_lanes_within_the_cer_bar(trained):
    from handwritten_ocr_amd import pipeline

    pipe = pipeline.LanePipeline(trained.eng, lanes=2)
    try:
        assert all(e.fp8_kv for e in pipe.engines)
        batches = [trained.reads(n) for n in (24, 8, 40, 24)]
        jobs = [(lambda e, hooks, p=p, q=q: e.generate(p, q, max_new=trained.n, hooks=hooks)) for _, p, q in batches]
        for _ in range(2):   # second pass: both lanes replay captured graphs
            out = pipe.run(jobs)
            for (idx, _, _), streams in zip(batches, out):
                trained.check(idx, streams, f"two lanes, batch of {len(idx)}")
    finally:
        pipe.close()


@pytest.mark.parametrize("family", ["qwen2_vl", "qwen2_5_vl"])
def test_the_drop_in_with_hwocr_kv_dtype_e4m3(family, tmp_path, monkeypatch, capsys):
    """tools.run_ocr / run_ocr_batch with HWOCR_KV_DTYPE=e4m3 in the environment: the engine the drop-in builds keeps an E4M3 cache."""
    from handwritten_ocr_amd import tools

    meta = trained_meta(family)
    monkeypatch.setenv("HWOCR_MODEL", trained_dir(family))
    monkeypatch.setenv("HWOCR_KV_DTYPE", "e4m3")
    monkeypatch.setenv("HWOCR_MAX_READS", "16")
    monkeypatch.setenv("HWOCR_CTX", "512")
    monkeypatch.setenv("HWOCR_KEEP_RESIDENT", "0")
    monkeypatch.setattr(tools, "_ocr_model", None)
    monkeypatch.setattr(tools, "_ocr_processor", None)
    paths = []
    for c in meta["cases"]:
        p = tmp_path / f"page{c['page_seed']}.png"
        Image.fromarray(trained_page(c), "RGB").save(p)
        paths.append(str(p))
    params = {"max_new_tokens": meta["max_new_tokens"]}
    hf = [c["hf_text"] for c in meta["cases"]]
    try:
        one = tools.run_ocr(paths[0], params)
        assert f"Running OCR on {os.path.basename(paths[0])}" in capsys.readouterr().out
        assert tools._ocr_model is not None and tools._ocr_model.fp8_kv and tools._ocr_model.k_cache.dtype == torch.uint8
        texts = tools.run_ocr_batch(paths, params)
        many = tools.run_ocr_batch(paths * 5, params)    # 40 reads through 16 slots over two lanes
    finally:
        tools.unload_ocr_model()
    assert one == texts[0]
    m, m5 = mean_cer(hf, texts), mean_cer(hf * 5, many)
    print(f"[e4m3 cache, trained {family}] drop-in: mean CER {m:.4f} (8 reads), {m5:.4f} (40 reads through 16 slots)")
    assert m <= CER_BAR and m5 <= CER_BAR, (m, m5)
