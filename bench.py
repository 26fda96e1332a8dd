#!/usr/bin/env python3
"""Headline benchmark: handwritten pages/sec (1024x1024 page, 3 preprocessing-strategy reads each) on MI355X.

One "step" = one pass of the read path over one batch of synthetic pages on every rank (page image ->
token ids -> merged text):
    raw RGB page (uint8 1024x1024x3, resident in HBM when the timed region starts)
    -> the 3 strategy chains + the image processor's bicubic resize on the device (gpupre.py; bit-identical to the
       reference's PIL path, ocr_agent/tools.py:633-673 + HF image_processing_pil_qwen2_vl.py:152-183)
    -> vision tower -> prefill -> N_out greedy tokens per read (min_new == max_new, so the work is fixed: random-init
       logits otherwise hit EOS at once) -> gather token streams to rank 0 -> per page compare_versions(read 1, read 2)
       + merge_versions(all reads).
Weights: random init at the Qwen2-VL-2B shape (no checkpoint is reachable offline).

    python bench.py --gpus N --steps K --warmup W      N > 1 without WORLD_SIZE: this process only spawns N ranks (one per
                                                       GPU, RCCL) and relays rank 0's line; it never touches the GPU itself
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...     (ranks made by the launcher)

A plain run does what the headline needs and no more: set up, warm up, time K steps, write --dump-outputs, print ONE JSON line
on rank 0 (contract in the task statement).  Beside `value` that line carries what the timed region's own events give:
    roofline      dominant kernel = gemm_wide (bf16 MFMA): algorithmic FLOPs / HIP-event time of its launches inside
                  the timed steps, against the 2.5 PFLOP/s dense bf16 peak
    phases_ms_per_step, decode_roofline   the lanes' phase times in the timed steps
--full adds every leg that takes runs of its own (over a minute more; --no-extras / --no-cpu-baseline leave parts of it out):
    with_upload, host_preprocess_path, single_page   the same step with the PCIe upload of the raw pages inside the clock, with
                  the reference's default host (PIL) preprocessing instead of the device path, and the single-page latency of
                  BASELINE config 2 as literally stated (one page, 3 reads)
    one_batch_at_a_time   (lanes > 1) one batch at a time; `roofline` is then taken from it: the kernel alone on the chip
    cpu_baseline  the CPU oracle (oracle/, a restatement of the HF arithmetic the reference runs) timed on this host: one whole
                  read at full depth on the engine's own weights, 32 decode steps measured and the rest scaled per token
                  (see `sample`); parity_full_depth_vs_oracle = the engine held to that very read, teacher-forced
    parity_vs_hf_goldens  the tiny HF goldens and the trained checkpoints of tests/golden read through the engine
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402

WORKLOAD_NAMES = {"paligemma-3b": "PaliGemma-3B (SigLIP-So400m 896 + Gemma-2B, bf16)", "qwen2-vl-2b": "Qwen2-VL-2B", "qwen2.5-vl-7b": "Qwen2.5-VL-7B / olmOCR-2-7B", "qwen2.5-vl-3b": "Qwen2.5-VL-3B"}
BF16_MFMA_PEAK_TFLOPS = 2500.0   # MI355X_MICROARCH.md: ~2.5 PF dense bf16
FP8_MFMA_PEAK_TFLOPS = 5000.0    # MI355X_MICROARCH.md: ~5 PF dense fp8 (block-scaled f8f6f4 MFMA forms)
HBM_PEAK_GBS = 8000.0


def synthetic_prompt(cfg, n_img: int) -> np.ndarray:
    """14 prefix ids + <vision_start> + image placeholders + <vision_end> + 16 suffix ids.
    PaliGemma: image placeholders + <bos> + 16 prompt ids (its processor's layout)."""
    rng = np.random.default_rng(0)
    if cfg.family == "paligemma":
        return np.asarray([cfg.image_token_id] * n_img + [cfg.bos_id] + rng.integers(3, 1000, size=16).tolist(), np.int32)
    pre = rng.integers(0, 1000, size=14).tolist()
    suf = rng.integers(0, 1000, size=16).tolist()
    return np.asarray(pre + [cfg.vision_start_id] + [cfg.image_token_id] * n_img + [cfg.vision_end_id] + suf, np.int32)


def wide_gemm_flops_per_read(cfg, hw: tuple[int, int], T: int) -> float:
    """ALGORITHMIC FLOPs of the Linears / patch conv that run as wide-GEMM launches for ONE read (SURVEY.md 8d's per-unit figure, the
    GEMM part of it): the model's own dimensions — patches and prompt tokens as they are, K = 3*tps*patch^2 for the patch conv, the
    tower MLP at its checkpoint width — not the padded ones the launches carry (rows rounded up to 64, K 1176 -> 1216, 3420 -> 3456)."""
    P = (hw[0] // cfg.patch_size) * (hw[1] // cfg.patch_size)
    d = cfg.embed_dim
    patch_k = 3 * cfg.tps * cfg.patch_size ** 2
    if cfg.family == "qwen2_vl":
        mlp = 2 * 2.0 * P * d * cfg.mlp_dim
    elif cfg.family == "qwen2_5_vl":
        mlp = 3 * 2.0 * P * d * cfg.vit_inter
    else:
        mlp = 2 * 2.0 * P * d * cfg.vit_inter
    vision = 2.0 * P * patch_k * d + cfg.depth * (2.0 * P * d * 4 * d + mlp)
    if cfg.family == "paligemma":
        vision += 2.0 * P * d * cfg.hidden                                   # the projector
    else:
        m, md = P // cfg.merge ** 2, d * cfg.merge ** 2
        vision += 2.0 * m * md * md + 2.0 * m * md * cfg.hidden              # the merger's two Linears
    hd = cfg.head_dim
    layer = 2.0 * T * cfg.hidden * (cfg.q_heads + 2 * cfg.kv_heads) * hd + 2.0 * T * cfg.q_heads * hd * cfg.hidden \
        + 3 * 2.0 * T * cfg.hidden * cfg.inter
    return vision + cfg.layers * layer


def strategies_for(reads_per_page: int) -> list:
    from handwritten_ocr_amd.compat import config

    return list(config.PREPROCESSING_STRATEGIES[:reads_per_page])


def target_hw(cfg, side: int) -> tuple[int, int]:
    from handwritten_ocr_amd import imageproc
    from handwritten_ocr_amd.compat import config

    if cfg.family == "paligemma":
        return cfg.image_size, cfg.image_size
    return imageproc.smart_resize(side, side, cfg.patch_size * cfg.merge, config.OCR_MIN_PIXELS, config.OCR_MAX_PIXELS)


def raw_pages(n_pages: int, seed0: int, side: int) -> list[np.ndarray]:
    """The step's input: synthetic handwritten pages as RGB uint8 arrays (what Image.open hands the reference)."""
    from handwritten_ocr_amd import synth

    return [np.ascontiguousarray(synth.make_page(seed0 + p, side, side)) for p in range(n_pages)]


def host_strategy_pages(cfg, raws: list, reads_per_page: int, device) -> tuple[list, float]:
    """The reference's default path for the same reads: PIL strategy chains + PIL bicubic resize on the host
    (preprocess.apply_strategy, imageproc.prepare_page), 8 threads, then one upload per read."""
    from concurrent.futures import ThreadPoolExecutor

    from PIL import Image

    from handwritten_ocr_amd import imageproc, preprocess
    from handwritten_ocr_amd.compat import config

    strategies = strategies_for(reads_per_page)

    def one(raw):
        img = Image.fromarray(raw, "RGB")
        out = []
        for s in strategies:
            pre = preprocess.apply_strategy(img, s, quiet=True)
            out.append(imageproc.prepare_square(pre, cfg.image_size) if cfg.family == "paligemma" else
                       imageproc.prepare_page(pre, cfg.patch_size, cfg.merge, config.OCR_MIN_PIXELS, config.OCR_MAX_PIXELS))
        return out

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=8) as pool:
        per_page = list(pool.map(one, raws))
    host_s = time.perf_counter() - t0
    return [torch.from_numpy(a.copy()).to(device) for page in per_page for a in page], host_s


def _host_threads() -> int:
    # the GPU box grants ~16 host cores per GPU; more torch threads than that only oversubscribe
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    threads = max(1, min(torch.get_num_threads(), avail, 16))
    torch.set_num_threads(threads)
    return threads


def _cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _strings_s() -> tuple[float, int]:
    from oracle import text_ref

    rng = np.random.default_rng(1)
    words = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, size=int(rng.integers(2, 9)))) for _ in range(260)]
    texts = [" ".join(words)] + [" ".join(w if rng.random() > 0.1 else w[::-1] for w in words) for _ in range(2)]
    t = time.perf_counter()
    text_ref.compare_versions(texts[0], texts[1])
    text_ref.merge_versions(texts)
    return time.perf_counter() - t, len(texts[0])


def cpu_baseline(cfg, sd_cpu: dict, raw_page: np.ndarray, strategy, n_out: int, reads_per_page: int, n_dec: int = 32) -> tuple[dict, dict]:
    """The reference's CPU path — processor -> generate -> slice (ocr_agent/tools.py:744-769) — restated (oracle/, bit-identical to
    HF's bf16 classes on the tiny goldens) and MEASURED on this host: ONE whole read at FULL depth and width of the SAME weights the
    engine holds (every tower block, every decoder layer, the full LM head), with the first `n_dec` decode steps timed and the
    remaining n_out - 1 - n_dec steps scaled per token (the cost per token is flat at these context lengths: BASELINE.md 2); x
    reads_per_page serial reads per page as nodes.py:86-110, + compare / merge of three page-length texts in pure Python.
    Returns (the cpu_baseline object, what the oracle computed for that read: prompt, page, tokens, per-step logits — the
    full-depth parity leg compares the engine with it)."""
    import torch.nn.functional as F
    from PIL import Image

    from handwritten_ocr_amd import imageproc, preprocess
    from handwritten_ocr_amd.compat import config

    threads = _host_threads()
    img = preprocess.apply_strategy(Image.fromarray(raw_page, "RGB"), strategy, quiet=True)
    n_dec = max(1, min(n_dec, n_out - 1))
    t0 = time.perf_counter()
    with torch.no_grad():
        if cfg.family == "paligemma":
            from oracle.paligemma_ref import PaliGemmaRef, PaliRefConfig

            ref = PaliGemmaRef(PaliRefConfig(
                v_layers=cfg.depth, v_hidden=cfg.embed_dim, v_heads=cfg.num_heads, v_inter=cfg.vit_inter, patch_size=cfg.patch_size,
                image_size=cfg.image_size, hidden=cfg.hidden, layers=cfg.layers, q_heads=cfg.q_heads, kv_heads=cfg.kv_heads,
                head_dim=cfg.head_dim, inter=cfg.inter, vocab=cfg.vocab, rope_theta=cfg.rope_theta, image_token_id=cfg.image_token_id,
                eos_ids=tuple(cfg.eos_ids), pad_id=cfg.pad_id), sd_cpu)
            lut = imageproc.pixel_lut((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
            page = imageproc.prepare_square(img, cfg.image_size)
            pv = torch.from_numpy(np.stack([lut[c][page[:, :, c]] for c in range(3)]))
            t_img = time.perf_counter() - t0
            emb = ref.vision(pv)
            t_vis = time.perf_counter() - t0 - t_img
            prompt = synthetic_prompt(cfg, emb.shape[0])
            ids = torch.from_numpy(prompt).long()
            mask = ids == cfg.image_token_id
            x = ref.embed(torch.where(mask, torch.zeros_like(ids), ids))
            x[mask] = emb.to(x.dtype)
            cache = [None] * cfg.layers
            last = ref.lm_head(ref.decoder(x, torch.arange(len(ids)) + 1, cache, bidirectional=True)[-1:])[0]
            step = lambda tok: ref.step(tok, cache)  # noqa: E731
        else:
            from oracle import image_ref
            from oracle.qwen2vl_ref import Qwen2VLRef, RefConfig, rope_index

            ref = Qwen2VLRef(RefConfig(
                depth=cfg.depth, embed_dim=cfg.embed_dim, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, family=cfg.family,
                vit_inter=cfg.vit_inter, window_size=cfg.window_size, fullatt=tuple(cfg.fullatt), hidden=cfg.hidden, layers=cfg.layers,
                q_heads=cfg.q_heads, kv_heads=cfg.kv_heads, inter=cfg.inter, vocab=cfg.vocab, tie=cfg.tie,
                image_token_id=cfg.image_token_id, vision_start_id=cfg.vision_start_id, vision_end_id=cfg.vision_end_id,
                eos_ids=tuple(cfg.eos_ids), pad_id=cfg.pad_id), sd_cpu)
            page = imageproc.prepare_page(img, cfg.patch_size, cfg.merge, config.OCR_MIN_PIXELS, config.OCR_MAX_PIXELS)
            pv, grid = image_ref.pixel_values(img, config.OCR_MIN_PIXELS, config.OCR_MAX_PIXELS)
            t_img = time.perf_counter() - t0
            emb = ref.vision(torch.from_numpy(pv), [grid])
            t_vis = time.perf_counter() - t0 - t_img
            prompt = synthetic_prompt(cfg, emb.shape[0])
            ids = torch.from_numpy(prompt).long()
            x = F.embedding(ids, ref.w("model.language_model.embed_tokens.weight")).clone()
            x[ids == cfg.image_token_id] = emb.to(x.dtype)
            pos3, delta = rope_index(ids, cfg.image_token_id, [grid], cfg.merge)
            cache = [None] * cfg.layers
            last = ref.lm_head(ref.decoder(x, pos3, cache)[-1:])[0]   # HF computes the head on every row and keeps this one
            step = lambda tok: ref.step(tok, cache, delta)  # noqa: E731
        t_pre = time.perf_counter() - t0 - t_img - t_vis
        toks, logits = [], []
        t1 = time.perf_counter()
        for n in range(n_dec + 1):                     # n_dec decode steps follow the prefill's token
            lf = last.float().clone()
            lf[list(cfg.eos_ids)] = -float("inf")      # min_new == max_new, as the timed GPU step
            logits.append(last)
            toks.append(int(torch.argmax(lf)))
            if n < n_dec:
                last = step(toks[-1])
        t_dec = (time.perf_counter() - t1) / n_dec
    t_str, n_chars = _strings_s()
    t_read = t_img + t_vis + t_pre + (n_out - 1) * t_dec
    t_page = reads_per_page * t_read + t_str
    out = {"value": 1.0 / t_page, "unit": "pages/s", "cores": threads, "cpu_model": _cpu_model(), "kind": "port",
           "sample": (f"oracle/ (torch CPU bf16 restatement of the HF {cfg.family} path run_ocr calls, tools.py:744-769) on this host, "
                      f"{threads} threads: ONE whole read at full depth ({cfg.depth} tower blocks, {cfg.layers} decoder layers, "
                      f"T={len(prompt)}, the engine's own weights) measured - image processor, tower, prefill, {n_dec} decode steps; "
                      f"the other {n_out - 1 - n_dec} decode steps scaled per token; x{reads_per_page} serial reads per page "
                      f"(nodes.py:86-110) + compare/merge of three {n_chars}-char reads in pure Python.  Nothing extrapolated in depth."),
           "seconds_per_page": t_page, "measured_cpu_seconds": time.perf_counter() - t0,
           "parts_s": {"image_processor": t_img, "vision": t_vis, "prefill": t_pre, "decode_per_token": t_dec, "strings": t_str}}
    return out, {"page": page, "prompt": prompt, "tokens": toks, "logits": torch.stack(logits)}


def hf_cpu_reference(cfg, sd_cpu: dict, raw_page: np.ndarray, strategy, ora: dict, n_out: int, reads_per_page: int, t_strings: float) -> dict:
    """SURVEY.md 8d's wording of the CPU baseline: run_ocr's call sequence (ocr_agent/tools.py:744-769: processor -> generate ->
    slice) against HF `transformers` itself — the library the reference's CPU path IS — on this host, bf16 as tools.py:707 forces,
    on the SAME weights, page and prompt as the oracle read of cpu_baseline, which it must reproduce token for token (the oracle is a
    restatement of these very classes).  Qwen2-VL family only.  The model is built on the meta device and given the engine's weights
    by reference (load_state_dict(assign=True): no second copy of 2 B parameters); the rotary inv_freq buffers are recomputed in fp32
    as from_pretrained leaves them.  Per-token times from a StoppingCriteria hook; the steps beyond the measured ones are scaled as
    in cpu_baseline.  Reported beside cpu_baseline (kind "port"), never a reason to lose the line."""
    import transformers
    from PIL import Image
    from transformers import Qwen2VLConfig, Qwen2VLForConditionalGeneration, StoppingCriteria, StoppingCriteriaList
    from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import Qwen2VLImageProcessorPil

    from handwritten_ocr_amd import preprocess
    from handwritten_ocr_amd.compat import config

    if cfg.family != "qwen2_vl" or int(cfg.mlp_ratio) != cfg.mlp_ratio:
        return {"skipped": f"family {cfg.family}: the HF leg is written for the benchmarked Qwen2-VL shape"}
    hcfg = Qwen2VLConfig(
        vision_config=dict(depth=cfg.depth, embed_dim=cfg.embed_dim, hidden_size=cfg.hidden, hidden_act="quick_gelu", mlp_ratio=int(cfg.mlp_ratio),
                           num_heads=cfg.num_heads, in_channels=3, patch_size=cfg.patch_size, spatial_merge_size=cfg.merge,
                           temporal_patch_size=cfg.tps),
        text_config=dict(vocab_size=cfg.vocab, hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=cfg.layers,
                         num_attention_heads=cfg.q_heads, num_key_value_heads=cfg.kv_heads, max_position_embeddings=32768,
                         rms_norm_eps=cfg.eps, tie_word_embeddings=bool(cfg.tie),
                         rope_parameters={"rope_type": "default", "rope_theta": cfg.rope_theta, "mrope_section": list(cfg.mrope_section)}),
        image_token_id=cfg.image_token_id, video_token_id=cfg.image_token_id + 1, vision_start_token_id=cfg.vision_start_id,
        vision_end_token_id=cfg.vision_end_id, tie_word_embeddings=bool(cfg.tie))
    t0 = time.perf_counter()
    with torch.device("meta"):
        model = Qwen2VLForConditionalGeneration(hcfg)
    res = model.load_state_dict(sd_cpu, strict=False, assign=True)
    if [k for k in res.missing_keys if k != "lm_head.weight"] or res.unexpected_keys:
        return {"error": f"state dict does not fit the HF model: missing {res.missing_keys[:3]}, unexpected {res.unexpected_keys[:3]}"}
    model.tie_weights()
    vis = model.model.visual.rotary_pos_emb
    dim = vis.inv_freq.shape[0] * 2
    vis.inv_freq = 1.0 / (10000.0 ** (torch.arange(0, dim, 2, dtype=torch.float) / dim))
    rot = model.model.language_model.rotary_emb
    hd = cfg.hidden // cfg.q_heads
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.int64).to(dtype=torch.float) / hd))
    rot.inv_freq, rot.original_inv_freq = inv, inv.clone()
    if any(b.is_meta for b in model.buffers()) or any(p_.is_meta for p_ in model.parameters()):
        return {"error": "a tensor of the HF model is still on the meta device"}
    model.eval()
    t_build = time.perf_counter() - t0
    img = preprocess.apply_strategy(Image.fromarray(raw_page, "RGB"), strategy, quiet=True)
    t0 = time.perf_counter()
    proc = Qwen2VLImageProcessorPil(min_pixels=config.OCR_MIN_PIXELS, max_pixels=config.OCR_MAX_PIXELS)
    px = proc(images=[img], return_tensors="pt")
    t_img = time.perf_counter() - t0
    ids = torch.from_numpy(np.asarray(ora["prompt"], np.int64))[None]
    n = len(ora["tokens"])
    stamps = []

    class Clock(StoppingCriteria):
        def __call__(self, input_ids, scores, **kw):
            stamps.append(time.perf_counter())
            return torch.zeros(input_ids.shape[0], dtype=torch.bool)

    model.generation_config.eos_token_id, model.generation_config.pad_token_id = list(cfg.eos_ids), cfg.pad_id
    t0 = time.perf_counter()
    with torch.no_grad():
        out = model.generate(input_ids=ids, pixel_values=px["pixel_values"].to(torch.bfloat16), image_grid_thw=px["image_grid_thw"],
                             mm_token_type_ids=(ids == cfg.image_token_id).int(), attention_mask=torch.ones_like(ids), do_sample=False,
                             max_new_tokens=n, min_new_tokens=n, stopping_criteria=StoppingCriteriaList([Clock()]))
    t_gen = time.perf_counter() - t0
    toks = out[0, ids.shape[1]:].tolist()
    t_first = stamps[0] - t0                                   # tower + prefill + the first token
    t_dec = (stamps[-1] - stamps[0]) / max(1, len(stamps) - 1)  # per decode step
    t_read = t_img + t_first + (n_out - 1) * t_dec
    t_page = reads_per_page * t_read + t_strings
    same = toks == list(ora["tokens"])
    return {"value": 1.0 / t_page, "unit": "pages/s", "cores": torch.get_num_threads(), "kind": "transformers on the CPU (the library the reference's CPU path runs)",
            "transformers": transformers.__version__, "seconds_per_page": t_page, "measured_cpu_seconds": t_img + t_gen,
            "parts_s": {"image_processor": t_img, "tower_prefill_first_token": t_first, "decode_per_token": t_dec, "model_build": t_build},
            "tokens_equal_to_the_oracle_read": bool(same), "first_difference": None if same else next(i for i, (a, b) in enumerate(zip(toks, ora["tokens"])) if a != b),
            "sample": f"HF Qwen2VLForConditionalGeneration.generate on this host's cores, bf16, full depth, the engine's own weights, T={ids.shape[1]}, "
                      f"{n} tokens measured ({n - 1} decode steps timed by a StoppingCriteria hook), the other {n_out - n} steps scaled per token; "
                      f"x{reads_per_page} serial reads per page + the same compare / merge seconds as cpu_baseline"}


def full_depth_parity(eng, ora: dict) -> dict:
    """The engine against the full-depth oracle read of cpu_baseline (same weights, same page, same prompt): teacher-forced logits
    of the first steps, as tests/test_fullwidth_oracle_gpu.py does at depth 2.  Reported, not asserted (the bench never fails on it)."""
    n = len(ora["tokens"])
    toks, lg = eng.generate([ora["page"]], [ora["prompt"]], max_new=n, min_new=n, forced=np.asarray([ora["tokens"]]), return_logits=True)
    got, want = lg[0].float().cpu(), ora["logits"].float()
    scale = max(1.0, float(want.abs().max()))
    d = (got - want).abs()
    top2 = want.topk(2, -1).values
    dec = (top2[:, 0] - top2[:, 1]) > 0.05
    same = torch.tensor([a == b for a, b in zip(toks[0], ora["tokens"])])
    return {"steps": n, "logit_scale": scale, "mean_abs_err_over_scale": float(d.mean()) / scale,
            "p999_abs_err_over_scale": float(d.flatten().quantile(0.999)) / scale, "max_abs_err_over_scale": float(d.max()) / scale,
            "decisive_steps": int(dec.sum()), "top1_agreement_on_decisive_steps": float((same & dec).sum()) / max(1, int(dec.sum())),
            "tolerance": "tests/test_model_gpu.py: mean <= 5e-3, p99.9 <= 3e-2, max <= 6e-2 (x scale); top-1 on decisive steps = 1",
            "note": "engine vs oracle/ at FULL depth and width on the bench's weights (random init), one read, teacher-forced"}


def parity_check(device) -> dict:
    """BASELINE's metric ends in "CER vs ref": the tiny seeded models of tests/golden (outputs of the real HF classes) through
    the same engine on this GPU — normalised edit distance of the greedy token stream against HF's and the teacher-forced
    logit error (random-init weights: a trained checkpoint is not reachable offline)."""
    from PIL import Image
    from safetensors.torch import load_file

    from handwritten_ocr_amd import engine, imageproc, text

    gold = os.path.join(ROOT, "tests", "golden")
    out = {}
    for fam, stem, preset in (("qwen2_vl", "qwen2vl_tiny", "tiny"), ("qwen2_5_vl", "qwen25vl_tiny", "tiny25")):
        try:
            cfg = engine.preset(preset)
            eng = engine.ReadEngine(cfg, load_file(os.path.join(gold, stem + "_weights.safetensors")), max_reads=4, ctx=256,
                                    device=str(device), vit_batch=2, prefill_batch=2)
            g = load_file(os.path.join(gold, stem + "_bf16.safetensors"))
            dist = toks = agree = decisive = 0
            worst = 0.0
            for case in ("a", "b"):
                page = imageproc.prepare_page(Image.fromarray(g[f"{case}.page"].numpy(), "RGB"), cfg.patch_size, cfg.merge,
                                              cfg.min_pixels, cfg.max_pixels)
                ids, hf = g[f"{case}.input_ids"].numpy(), g[f"{case}.greedy_tokens"].tolist()
                free = eng.generate([page], [ids], max_new=len(hf), min_new=len(hf))[0]
                dist += text.levenshtein("".join(chr(256 + t) for t in free), "".join(chr(256 + t) for t in hf))
                toks += len(hf)
                _, lg = eng.generate([page], [ids], max_new=len(hf), min_new=len(hf), forced=np.asarray([hf]), return_logits=True)
                want = g[f"{case}.step_logits"].float()
                worst = max(worst, float((lg[0].float().cpu() - want).abs().max()) / max(1.0, float(want.abs().max())))
                top2 = want.topk(2, -1).values
                dec = (top2[:, 0] - top2[:, 1]) > 0.05
                same = lg[0].float().cpu().argmax(-1) == want.argmax(-1)
                decisive += int(dec.sum())
                agree += int((same & dec).sum())
            eng.close()
            out[fam] = {"teacher_forced_top1_agreement_on_decisive_steps": agree / max(1, decisive), "decisive_steps": decisive,
                        "teacher_forced_logit_err_over_scale": worst, "free_running_token_edit_rate": dist / toks, "tokens": toks,
                        "note": "random-init weights: near-tied logits make free-running streams diverge after the first "
                                "flipped near-tie (reported only); the pinned quantities are the teacher-forced ones"}
        except Exception as e:  # a report, never a reason to lose the measurement
            out[fam] = {"error": f"{type(e).__name__}: {e}"}
    out["trained_cer"] = trained_cer(device)
    return out


def trained_cer(device) -> dict:
    """The accuracy bar itself (`north_star`: output CER within 0.5 % of the reference's; metric = cer(), ocr_agent/tools.py:103-118,
    over the text generate() returns, tools.py:764-769): tests/golden/trained_* hold HF's own free-running transcriptions of 8
    synthetic pages by a briefly TRAINED tiny checkpoint (decisive greedy choices; tools/make_goldens.py::make_trained).  The engine
    reads the same pages free-running — 8 reads (the <= 16-read decode chain) and 252 reads (the bench's decode geometry) — and the
    mean CER of its text against HF's is reported (asserted <= 0.005 by tests/test_trained_gpu.py)."""
    from PIL import Image

    from handwritten_ocr_amd import engine, synth, text, tokenizer
    from handwritten_ocr_amd.compat import config

    gold = os.path.join(ROOT, "tests", "golden")
    out = {"bar": 0.005, "metric": "mean over pages of cer(HF text, engine text)"}
    for fam, stem in (("qwen2_vl", "trained_qwen2vl"), ("qwen2_5_vl", "trained_qwen25vl"), ("paligemma", "trained_paligemma")):
        try:
            with open(os.path.join(gold, stem + ".json"), encoding="utf-8") as f:
                meta = json.load(f)
            ckpt = os.path.join(gold, stem)
            cfg, sd = engine.load_checkpoint_dir(ckpt, device=str(device))
            cfg.min_pixels, cfg.max_pixels = config.OCR_MIN_PIXELS, config.OCR_MAX_PIXELS
            eng = engine.ReadEngine(cfg, sd, max_reads=252, ctx=512, device=str(device), vit_batch=12, prefill_batch=16)
            proc = tokenizer.Processor(cfg, tokenizer.HFTokenizer(cfg, ckpt), template_dir=ckpt)
            cases = meta["cases"]
            prep = [proc.prepare(Image.fromarray(synth.tint_page(synth.make_page(c["page_seed"], *c["page_hw"]), c["page_tint"]), "RGB"),
                                 meta["prompt"]) for c in cases]
            res = {}
            for reads in (8, 252):
                idx = [i % len(cases) for i in range(reads)]
                streams = eng.generate([prep[i][0] for i in idx], [prep[i][1] for i in idx], max_new=meta["max_new_tokens"])
                texts = [proc.decode(t, skip_special_tokens=True) for t in streams]
                res[f"{reads}_reads"] = {"mean_cer": sum(text.cer(cases[i]["hf_text"], t) for i, t in zip(idx, texts)) / reads,
                                         "token_streams_differing_from_hf": sum(t != cases[i]["hf_tokens"] for i, t in zip(idx, streams))}
            eng.close()
            out[fam] = dict(res, pages=len(cases), new_tokens=meta["max_new_tokens"],
                            decisive_fraction_margin_gt_1=meta["decisive_fraction_margin_gt_1"])
        except Exception as e:
            out[fam] = {"error": f"{type(e).__name__}: {e}"}
    return out


def dump_outputs(out_dir: str, gathered: list, compared: list, merged: list) -> None:
    """--dump-outputs: what the timed path handed its caller in its last timed step, as float arrays that two builds of the project
    can be compared with (the inputs are seeded, so the same arguments give the same inputs).  Token ids and code points are below
    2^24, exact in float32; the whole dump is a few MB at the default shape (<= 256 reads x 512 tokens per rank).
        tokens.npy             [reads of every rank, new_tokens]  greedy token streams, rank-major (the gather on rank 0)
        token_counts.npy       [reads of every rank]              stream lengths the gather carried
        merged_text.npy        [pages, max_len]                   merge_versions of each page of rank 0, code points, -1 padded
        merged_len.npy         [pages]                            their lengths
        compare_versions.npy   [pages, 3]                         agreement_rate, char_edit_distance, word_edit_distance of
                                                                  reads 1 and 2 of each page of rank 0 (absent with --reads 1)"""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"tokens": np.concatenate([t.cpu().numpy() for t, _ in gathered]).astype(np.float32),
              "token_counts": np.concatenate([c.cpu().numpy() for _, c in gathered]).astype(np.float32),
              "merged_len": np.asarray([len(m) for m in merged], np.float32)}
    codes = np.full((len(merged), max([len(m) for m in merged] + [1])), -1.0, np.float32)
    for i, m in enumerate(merged):
        codes[i, : len(m)] = [ord(ch) for ch in m]
    arrays["merged_text"] = codes
    if compared:
        arrays["compare_versions"] = np.asarray([[c["agreement_rate"], c["char_edit_distance"], c["word_edit_distance"]]
                                                 for c in compared], np.float64)
    if sum(a.nbytes for a in arrays.values()) > 64 << 20:
        raise SystemExit(f"--dump-outputs: {sum(a.nbytes for a in arrays.values())} bytes exceed the 64 MB bound")
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def spawn_ranks(n: int, argv: list[str]) -> int:
    """`python bench.py --gpus N` without a launcher: start N copies of this script, one per GPU, with the rendezvous
    variables torch.distributed.run would set, wait, and relay rank 0's JSON line.  This parent makes no GPU call (a
    process that has initialised the GPU must not fork workers or be replaced): children are fresh interpreters."""
    import socket
    import subprocess

    with socket.socket() as sk:  # a free rendezvous port
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    # rank 0's stdout is read by a thread while every rank is watched: a rank that dies would leave the others waiting in a
    # collective until the RCCL timeout, so the remaining ranks (these exact child processes) are terminated instead
    import threading

    chunks: list = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    failed = False
    while any(p.poll() is None for p in procs):
        if any(p.poll() not in (None, 0) for p in procs):
            failed = True
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            break
        time.sleep(0.5)
    codes = []
    for p in procs:
        try:
            codes.append(p.wait(timeout=30))
        except subprocess.TimeoutExpired:
            p.kill()
            codes.append(p.wait())
    reader.join(timeout=10)
    out0 = chunks[0] if chunks else ""
    lines = [] if failed else [l for l in (out0 or "").splitlines() if l.startswith("{")]
    if lines:
        print(lines[-1], flush=True)
    rc = next((c for c in codes if c), 0)
    if rc:
        sys.stderr.write(f"bench.py: rank exit codes {codes}\n")
    return rc


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pages", type=int, default=84, help="pages per step per GPU (x3 reads in flight, <= 256 reads)")
    ap.add_argument("--reads", type=int, default=3)
    ap.add_argument("--new-tokens", type=int, default=512)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--model", default="qwen2-vl-2b")
    ap.add_argument("--vit-batch", type=int, default=12)
    ap.add_argument("--prefill-batch", type=int, default=16)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the legs beside the headline: with_upload, one_batch_at_a_time, "
                         "host_preprocess_path, single_page, cpu_baseline, parity_full_depth_vs_oracle, parity_vs_hf_goldens")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines and the parity legs")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the with_upload / one_batch_at_a_time / host_preprocess_path / single-page legs")
    ap.add_argument("--profile-steps", type=int, default=0, help="(ignored: every wide-GEMM launch of the timed region carries HIP events)")
    ap.add_argument("--lanes", type=int, default=2,
                    help="batches in flight on the GPU, one engine lane, host thread and HIP stream each (pipeline.LanePipeline); "
                         "1 = one batch at a time (the schedule of rounds 1-2)")
    ap.add_argument("--lane-order", default="lockstep", choices=("lockstep", "alternate"),
                    help="lockstep: the lanes start together (tower beside tower, decode beside decode); alternate: batch k's decode "
                         "beside batch k+1's tower + prefill, enforced by events (measured slower: pipeline.py)")
    ap.add_argument("--fp8", action="store_true",
                    help="E4M3 wide GEMMs for the vision tower and the prefill (BASELINE config 4; not the headline configuration)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed to DIR/<name>.npy (rank 0; see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    extras_on = args.full and not args.no_extras          # the legs that take runs of their own beside the timed steps
    cpu_on = args.full and not args.no_cpu_baseline

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))

    from handwritten_ocr_amd import _lib, engine, gpupre, pipeline, shard, text, tokenizer

    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world_env}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (the read engine has no CPU path)")
    rank, local, world = shard.init_from_env()
    dev = torch.device(f"cuda:{shard.local_device_index(local)}")
    torch.cuda.set_device(dev)
    import torch.distributed as dist

    cfg = engine.preset(args.model)
    n_reads = args.pages * args.reads
    strategies = strategies_for(args.reads)
    if not all(gpupre.supported(s) for s in strategies):
        raise SystemExit("OpenCV is importable here: the reference takes its cv2 branches, which the device preprocessing does not "
                         "restate (parity unpinned) — run without cv2")
    sd = engine.random_state_dict(cfg, seed=0, device=dev)
    # KV-cache length: prompt (image tokens + ~32) + generated tokens, rounded up
    hw = target_hw(cfg, args.side)
    n_img_tokens = (hw[0] // cfg.patch_size) * (hw[1] // cfg.patch_size) // cfg.merge ** 2
    ctx = 2048 if n_img_tokens + 64 + args.new_tokens <= 2048 else (n_img_tokens + 128 + args.new_tokens + 63) // 64 * 64
    eng = engine.ReadEngine(cfg, sd, max_reads=n_reads, ctx=ctx, device=str(dev), vit_batch=args.vit_batch,
                            prefill_batch=args.prefill_batch, fp8=args.fp8)
    if not (world_env == 1 and cpu_on):
        del sd  # (else kept: the CPU baseline runs the oracle on a host copy of these very weights; the engine aliases them)
    eng.collect_timings = True
    tok = tokenizer.ByteTokenizer(cfg, fold_unknown=True)
    pipe = pipeline.LanePipeline(eng, lanes=max(1, args.lanes), order=args.lane_order)
    for e in pipe.engines:
        e.collect_timings = True
    sps = {id(e): gpupre.StrategyPages(dev) for e in pipe.engines}   # (a lane's own scratch: two host threads preprocess side by side)
    sp = sps[id(eng)]
    raws = raw_pages(args.pages, 1000 * rank, args.side)                    # host memory (what Image.open returns)
    raws_dev = [torch.from_numpy(r).to(dev) for r in raws]                   # the step's input, resident in HBM
    prompts = [synthetic_prompt(cfg, n_img_tokens)] * n_reads
    lib = _lib.hip()

    # world > 1 with lanes: a lane's host thread issues no collective (RCCL wants every rank to issue its collectives in ONE order from
    # ONE thread); the lanes hand each finished step's token streams to this rank's gather thread, which gathers + merges them in step
    # order WHILE the lanes read the next steps (inside the timed region, as with one GPU, where the lane threads merge)
    import threading
    deferred, deferred_cv = {}, threading.Condition()
    # --dump-outputs: (gathered token streams, compare_versions results, merged texts) of step `record["j"]` of the timed run_steps
    record = {"j": None, "out": None}

    def gather_and_merge(toks, n_pages, j=None):
        t = torch.tensor(toks, dtype=torch.int32, device=dev)
        counts = torch.full((len(toks),), args.new_tokens, dtype=torch.int32, device=dev)
        gathered = shard.gather_token_streams(t, counts, dst=0)
        merged, compared = [], []
        for p in range(n_pages):
            reads = [tok.decode(toks[p * args.reads + r]) for r in range(args.reads)]
            if len(reads) >= 2:
                compared.append(text.compare_versions(reads[0], reads[1]))
            merged.append(text.merge_versions(reads))
        if j is not None and j == record["j"] and gathered is not None:
            record["out"] = (gathered, compared, merged)
        return merged

    def read_and_merge(pages, n_pages, e=None, hooks=None, j=None):
        e = e or eng
        toks = e.generate(pages, prompts[: len(pages)], max_new=args.new_tokens, min_new=args.new_tokens, hooks=hooks)
        if hooks is not None and world > 1:
            with deferred_cv:
                deferred[hooks.k] = toks
                deferred_cv.notify_all()
            return None
        return gather_and_merge(toks, n_pages, j)

    def step(src=None, e=None, hooks=None, j=None):
        """One step on engine (lane) e.  src: device-resident raw pages (the timed configuration) or host arrays (upload inside the
        step).  Returns the lane's phase times of this step."""
        e = e or eng
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pages = [im for raw in (raws_dev if src is None else src) for im in sps[id(e)].pages(raw, strategies, hw)]
        e1.record()
        read_and_merge(pages, args.pages, e, hooks, j)
        return dict(e.timings, preprocess_ms=e0.elapsed_time(e1))   # (both events long complete: generate synchronised its stream)

    def run_steps(k, src=None):
        """k steps through the lanes (lanes == 1: one after the other on this thread's stream): their phase times in step order."""
        jobs = [(lambda e, hooks, src=src, j=j: step(src, e, hooks, j)) for j in range(k)]
        if world == 1 or len(pipe.engines) == 1 or k <= 1:
            return pipe.run(jobs)
        failed, bad_ranks = [], []

        def gather_in_step_order():
            torch.cuda.set_device(dev)
            for j in range(k):
                with deferred_cv:
                    deferred_cv.wait_for(lambda: j in deferred or failed)
                    toks = deferred.pop(j, None)   # None: a lane of THIS rank raised (pipe.run re-raises it below)
                # every rank says whether it has step j's streams BEFORE the data collective: a rank whose lane raised still takes part
                # in this one, and the others stop here instead of waiting in the gather until the backend's timeout
                bad = shard.failed_ranks(toks is not None, dev)
                if bad:
                    bad_ranks.extend(bad)
                    return
                gather_and_merge(toks, args.pages, j)

        th = threading.Thread(target=gather_in_step_order, name="hwocr-gather")
        th.start()
        try:
            out = pipe.run(jobs)
        except BaseException:
            with deferred_cv:
                failed.append(True)
                deferred_cv.notify_all()
            raise
        finally:
            th.join()
        if bad_ranks:
            raise RuntimeError(f"rank(s) {sorted(set(bad_ranks))} failed in their reads; rank {rank} stops with them")
        return out

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # W untimed warm-up steps; every lane must have run once (its decode graph is captured on its first batch), so with more lanes
    # than W the warm-up is lanes steps long
    warm = max(args.warmup, len(pipe.engines)) if args.warmup > 0 else 0
    if warm:
        run_steps(warm)
    barrier()
    # HIP events around every wide-GEMM launch of the whole timed region (a few microseconds per launch: 0.2 % of a step)
    _lib.check(lib.hwocr_profile_enable(2 if args.fp8 else 1))
    record["j"] = args.steps - 1 if args.dump_outputs else None
    t0 = time.perf_counter()
    phases = run_steps(args.steps)
    barrier()
    elapsed = time.perf_counter() - t0
    record["j"] = None   # (the legs below run steps of their own)
    prof_steps, t_prof = args.steps, elapsed
    ms, fl, n = C.c_double(), C.c_double(), C.c_long()
    _lib.check(lib.hwocr_profile_read(C.byref(ms), C.byref(fl), C.byref(n)))
    lib.hwocr_profile_enable(0)
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax)

    # ---- legs outside `value` (--full; rank 0, N = 1 only): the same step with the raw pages uploaded inside the clock, with the
    # reference's default host preprocessing, and BASELINE config 2 as literally stated (one page, its 3 reads in flight)
    extras = {}
    solo = world == 1 and extras_on
    if solo:
        k_up = max(2, 2 * len(pipe.engines))
        torch.cuda.synchronize()
        t = time.perf_counter()
        run_steps(k_up, raws)
        torch.cuda.synchronize()
        up_s = (time.perf_counter() - t) / k_up
        extras["with_upload"] = {"value": args.pages / up_s, "unit": "pages/s", "ms_per_step": up_s * 1e3, "steps": k_up,
                                 "note": "the timed schedule with the raw pages starting in host memory (pageable): 3 MB per page over "
                                         "PCIe inside the clock"}
    if len(pipe.engines) > 1 and extras_on:
        # one batch at a time on one stream (the schedule of rounds 1-2): what the overlap buys, the phase times of a batch that
        # has the chip to itself, and the dominant kernel's rate when nothing runs beside it.  Run on EVERY rank at every --gpus N
        # (the step's token gather is a collective): `roofline` then means the same thing in a BENCH line and in a SCALE line —
        # the kernel alone on rank 0's chip — instead of silently becoming the two-lane in-region figure for N > 1
        _lib.check(lib.hwocr_profile_enable(2 if args.fp8 else 1))
        torch.cuda.synchronize()
        t = time.perf_counter()
        seq = [step() for _ in range(2)]
        torch.cuda.synchronize()
        seq_s = (time.perf_counter() - t) / 2
        ms1, fl1, n1 = C.c_double(), C.c_double(), C.c_long()
        _lib.check(lib.hwocr_profile_read(C.byref(ms1), C.byref(fl1), C.byref(n1)))
        lib.hwocr_profile_enable(0)
        extras["one_batch_at_a_time"] = {
            "value": args.pages / seq_s, "unit": "pages/s", "ms_per_step": seq_s * 1e3,
            "phases_ms_per_step": {k[:-3]: float(np.mean([p[k] for p in seq])) for k in ("preprocess_ms", "vision_ms", "prefill_ms", "decode_ms")},
            "dominant_kernel_alone": {"achieved": fl1.value / (ms1.value * 1e-3) / 1e12 if ms1.value > 0 else 0.0, "unit": "TFLOP/s",
                                      "avg_launch_ms": ms1.value / max(1, n1.value), "launches": int(n1.value)},
            "note": "--lanes 1: tower, prefill, decode of one batch back to back on one stream"}
    if solo:
        t = time.perf_counter()
        host_pages, host_s = host_strategy_pages(cfg, raws, args.reads, dev)
        same = all(torch.equal(a, b) for a, b in zip(host_pages[: 4 * args.reads],
                                                     [im for raw in raws_dev[:4] for im in sp.pages(raw, strategies, hw)]))
        read_and_merge(host_pages, args.pages)
        torch.cuda.synchronize()
        hp_s = time.perf_counter() - t
        extras["host_preprocess_path"] = {"value": args.pages / hp_s, "unit": "pages/s", "ms_per_step": hp_s * 1e3,
                                          "host_preprocess_s_per_page": host_s / args.pages, "threads": 8,
                                          "identical_to_device_path": bool(same),
                                          "note": "PIL strategy chains + PIL bicubic on 8 host threads, then the same engine pass"}
        del host_pages
        one = [im for im in sp.pages(raws_dev[0], strategies, hw)]
        lat = []
        for _ in range(4):  # the first pass captures the 3-read decode graph
            torch.cuda.synchronize()
            t = time.perf_counter()
            pg = [im for im in sp.pages(raws_dev[0], strategies, hw)]
            read_and_merge(pg, 1)
            torch.cuda.synchronize()
            lat.append((time.perf_counter() - t) * 1e3)
        del one
        extras["single_page"] = {"latency_ms": float(np.median(lat[1:])), "pages_per_s": 1e3 / float(np.median(lat[1:])),
                                 "reads_in_flight": args.reads, "phases_ms": dict(eng.timings),
                                 "decode_ms_per_token": eng.timings.get("decode_ms", 0.0) / max(1, args.new_tokens - 1),
                                 "note": "BASELINE config 2 as literally stated: one 1024x1024 page, its 3 strategy reads in flight"}
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank != 0:
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, *record["out"])

    pages_total = args.pages * world * args.steps
    value = pages_total / elapsed
    # The dominant kernel's rate.  With one batch at a time: HIP events around every launch of the timed region.  With several lanes
    # two launches share the chip, so a launch's duration in the timed region is not the kernel's speed (it measures about half of
    # it); the roofline is then taken from the launches of the one-batch-at-a-time leg — the same events, the same workload, the
    # kernel alone on the chip — and the timed region's own figure is reported beside it (in_timed_region).
    in_region = {"achieved": fl.value / (ms.value * 1e-3) / 1e12 if ms.value > 0 else 0.0, "unit": "TFLOP/s",
                 "avg_launch_ms": ms.value / max(1, n.value), "launches": int(n.value),
                 "note": "HIP events over the timed region; with lanes > 1 two launches run side by side and share the CUs"}
    alone_leg = extras.get("one_batch_at_a_time", {}).get("dominant_kernel_alone")
    if len(pipe.engines) > 1 and alone_leg:
        achieved, roof_ms, roof_n, roof_where = alone_leg["achieved"], alone_leg["avg_launch_ms"] * alone_leg["launches"], alone_leg["launches"], \
            "one_batch_at_a_time leg (2 steps after the timed region): the kernel alone on the chip"
        roof_steps, roof_wall = 2, extras["one_batch_at_a_time"]["ms_per_step"] * 2e-3
    else:
        achieved, roof_ms, roof_n, roof_where = in_region["achieved"], ms.value, int(n.value), "the timed region" + (
            " (two lanes share the chip: --full measures the kernel alone)" if len(pipe.engines) > 1 else "")
        roof_steps, roof_wall = prof_steps, t_prof
    mean = lambda k: float(np.mean([p[k] for p in phases]))  # noqa: E731
    T = len(prompts[0])
    # `achieved` = ALGORITHMIC FLOPs (the model's own dimensions, wide_gemm_flops_per_read) of the sampled steps / the HIP-event time
    # of their wide-GEMM launches; the launches themselves carry ~1 % more (rows padded to 64, K 1176 -> 1216): issued_over_algorithmic
    alg_per_step = n_reads * wide_gemm_flops_per_read(cfg, hw, T)
    issued = (alone_leg["achieved"] * 1e12 * roof_ms * 1e-3) if (len(pipe.engines) > 1 and alone_leg) else fl.value
    achieved = alg_per_step * roof_steps / (roof_ms * 1e-3) / 1e12 if roof_ms > 0 else 0.0
    in_region["achieved"] = alg_per_step * prof_steps / (ms.value * 1e-3) / 1e12 if ms.value > 0 else 0.0
    dec_ms = mean("decode_ms") / max(1, args.new_tokens - 1)
    # the decode roofline is a statement about the decode kernels: taken from a batch that has the chip to itself when one was run
    alone = extras.get("one_batch_at_a_time", {}).get("phases_ms_per_step")
    dec_alone_ms = (alone["decode"] if alone else mean("decode_ms")) / max(1, args.new_tokens - 1)
    # decoder bytes per step: all layer weights + LM head (tied) + KV of every read at its mean context
    hd = cfg.head_dim
    per_layer = (cfg.q_heads + 2 * cfg.kv_heads) * hd * cfg.hidden + cfg.q_heads * hd * cfg.hidden + 3 * cfg.inter * cfg.hidden
    w_bytes = 2.0 * (cfg.layers * per_layer + cfg.vocab * cfg.hidden)
    kv_bytes = n_reads * cfg.layers * 2 * cfg.kv_heads * hd * 2 * (T + args.new_tokens / 2)
    # HBM-side traffic of the dominant kernel: not measurable in-process — taken from the committed summary of separate
    # `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes (tools/pmc_summary.py, corrections stated there)
    mfma_peak = FP8_MFMA_PEAK_TFLOPS if args.fp8 else BF16_MFMA_PEAK_TFLOPS
    traffic = None
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic_fp8.json" if args.fp8 else "pmc_traffic.json")) as f:
            traffic = json.load(f)["kernels"]["gemm_wide256_kernel_fp8" if args.fp8 else "gemm_wide256_kernel"]["traffic_bytes"]
    except (OSError, KeyError, ValueError):
        pass
    out = {
        "metric": "handwritten pages/sec (1024x1024, 3-strategy reads)", "value": value, "unit": "pages/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "fp8-e4m3 wide GEMMs (vision tower + prefill), bf16 elsewhere" if args.fp8 else "bf16", "data": "synthetic",
        "config": {"workload": f"{WORKLOAD_NAMES.get(cfg.name, cfg.name)} shape (random init) x {args.side}x{args.side} synthetic handwritten pages, "
                               f"{args.reads} preprocessing-strategy reads per page, {args.new_tokens} greedy tokens per read",
                   "strategies": [s if isinstance(s, str) else list(s) for s in strategies],
                   "strategies_note": "without OpenCV (neither image has it) the reference's deskew is the identity (tools.py:572), so "
                                      "strategies 0 and 1 hand the model identical pixels; ALL reads are computed all the same - "
                                      f"{n_reads} tower passes, prefills and decodes per step, nothing is deduplicated or cached",
                   "input_residency": "value: raw pages resident in HBM when the clock starts (the measurement contract of this "
                                      "bench); with_upload: the same step with the pages starting in host memory (SURVEY 8d's "
                                      "'PIL image in host memory'), 3 MB per page over PCIe inside the clock",
                   "timed_region": "raw RGB page resident in HBM -> strategy preprocessing + bicubic resize (device) -> vision tower -> "
                                   "prefill -> decode -> token gather -> compare/merge on the host",
                   "pages_per_step_per_gpu": args.pages, "reads_in_flight": n_reads, "prompt_tokens": T,
                   "image_tokens": int((prompts[0] == cfg.image_token_id).sum()), "new_tokens": args.new_tokens,
                   "single_page_latency_ms": extras.get("single_page", {}).get("latency_ms"),
                   "lanes": len(pipe.engines),
                   "schedule": (f"{len(pipe.engines)} batches in flight per GPU, one engine lane + host thread + HIP stream each, order "
                                f"'{pipe.order}' (pipeline.LanePipeline; same tokens as one batch at a time)" if len(pipe.engines) > 1 else
                                "one batch at a time: tower, prefill, decode back to back on one stream"),
                   "parallelism": f"replicas x{world}, pages sharded, RCCL gather of token streams"},
        "roofline": {"bound": "mfma",
                     "kernel": ("gemm_wide256_kernel<FP8> (E4M3 256x256x128 MFMA GEMM on v_mfma_f32_16x16x128_f8f6f4, 8 waves, staggered phases)"
                                if args.fp8 else "gemm_wide256_kernel / gemm_wide256w4_kernel (bf16 256x256x64 MFMA GEMM: 8 waves of 128x64 with staggered phases, or 4 waves "
                                     "of 128x128 where that form measures faster - HWOCR_GEMM256; every hwocr_gemm_wide launch is timed)"),
                     "achieved": achieved, "peak": mfma_peak, "unit": "TFLOP/s",
                     "frac": achieved / mfma_peak, "traffic": traffic, "measured_in": roof_where, "in_timed_region": in_region,
                     "traffic_note": "bytes per launch from profiles/pmc_traffic%s.json (separate rocprofv3 --pmc passes)" % ("_fp8" if args.fp8 else ""),
                     "sampled_steps": roof_steps, "launches": int(roof_n), "launches_per_step": int(roof_n) / roof_steps,
                     "avg_launch_ms": roof_ms / max(1, roof_n),
                     "algorithmic_flops_per_launch": alg_per_step * roof_steps / max(1, roof_n),
                     "algorithmic_flops_per_read": alg_per_step / n_reads,
                     "issued_over_algorithmic": issued / (alg_per_step * roof_steps) if roof_n else None,
                     "share_of_step_time": roof_ms / (roof_wall * 1e3)},
        "phases_ms_per_step": {"preprocess": mean("preprocess_ms"), "vision": mean("vision_ms"), "prefill": mean("prefill_ms"),
                               "decode": mean("decode_ms"), "decode_per_token": dec_ms,
                               "note": ("wall time of each phase of a batch WHILE the other lane's batch shares the chip (they overlap: the "
                                        "sum exceeds ms_per_step); one_batch_at_a_time (--full) has the phases of a batch alone"
                                        if len(pipe.engines) > 1 else "one batch at a time")},
        "decode_roofline": {"bound": "hbm", "bytes_per_step": w_bytes + kv_bytes, "achieved": (w_bytes + kv_bytes) / (dec_alone_ms * 1e-3) / 1e9,
                            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": (w_bytes + kv_bytes) / (dec_alone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                            "ms_per_token": dec_alone_ms, "measured": "decode of a batch alone on the chip" if alone else "timed region"},
    }
    out.update(extras)
    if world == 1 and cpu_on:
        try:
            sd_cpu = {k: v.to("cpu") for k, v in engine.normalize_keys(sd).items()}
            del sd
            out["cpu_baseline"], ora = cpu_baseline(cfg, sd_cpu, raws[0], strategies[0], args.new_tokens, args.reads)
            try:  # the same read through HF transformers itself on the same cores (SURVEY 8d's wording), token for token
                out["cpu_baseline"]["hf_transformers"] = hf_cpu_reference(cfg, sd_cpu, raws[0], strategies[0], ora, args.new_tokens, args.reads,
                                                                          out["cpu_baseline"]["parts_s"]["strings"])
            except Exception as e:
                out["cpu_baseline"]["hf_transformers"] = {"error": f"{type(e).__name__}: {e}"}
            del sd_cpu
            try:  # the same read through the engine, teacher-forced: full-depth, full-width parity on the bench's own weights
                out["parity_full_depth_vs_oracle"] = full_depth_parity(eng, ora)
            except Exception as e:
                out["parity_full_depth_vs_oracle"] = {"error": f"{type(e).__name__}: {e}"}
        except Exception as e:  # the baseline is a report, never a reason to lose the GPU measurement
            out["cpu_baseline"] = {"value": None, "unit": "pages/s", "cores": torch.get_num_threads(), "kind": "port",
                                   "sample": f"failed: {type(e).__name__}: {e}"}
        del eng, raws_dev
        torch.cuda.empty_cache()
        out["parity_vs_hf_goldens"] = parity_check(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
