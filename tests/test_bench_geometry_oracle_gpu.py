"""The engine against the CPU oracle at the geometry bench.py runs: engines built as the bench builds them (max_reads=252, vit_batch=12,
prefill_batch=16, ctx 2048 for Qwen and 4352 for PaliGemma), full-width presets at two tower blocks and two decoder layers,
random-init weights (engine.random_state_dict(seed=0)).

tests/test_fullwidth_oracle_gpu.py pins the same widths with <= 16 reads in flight, where a decode step takes the gemm_rows16 layer
and the prefill is one launch.  Here every read count is the bench's or above 16, so the decode takes the general layer
(gemm_stream GEMMs, one attention pass at 252 reads, split attention + merge below), and the prefill runs in 16-read chunks, most at
seq0 > 0.  What makes the composition visible, not only each kernel:

  * distinct pages (>= 12 per tower launch) of three grids - square, portrait, a small landscape page - mixed inside every prefill
    chunk, so the reads of a chunk differ in image-token count and M-RoPE rope_delta;
  * ragged prompts: a distinct text tail per read, the longest filling the cache to within max_new of ctx, the shortest a small page
    with no tail (most of its padded prompt rows empty);
  * a distinct teacher-forced token stream per read over N_NEW = 72 steps, so every read's decode crosses a 64-key tile and a 32-key
    E4M3 block boundary;
  * oracle reads chosen at the chunk seams: first and last of chunk 0, first of chunk 1, one in the middle chunk, the last read of
    the final partial chunk, the longest and the shortest prompt, every page grid.

The E4M3 KV cache (fp8_kv=True, bf16 weights) runs the same reads against the oracle's kv_quant hook (oracle/qwen2vl_ref.py).
Tolerances are the suite's (tests/_parity.py).  Every case asserts through engine.decode_plan which decode layer it runs."""
import dataclasses
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from tests._parity import check_logits

pytestmark = pytest.mark.gpu

N_NEW = 72
BENCH = dict(max_reads=252, vit_batch=12, prefill_batch=16)
# Qwen reads: read r shows page (r // 3) % 12 of grid r % 3.  ORACLE_QWEN: 0 / 15 first and last of prefill chunk 0, 16 first of
# chunk 1, 117 in the middle chunk (7), 251 the last read of the final, partial chunk (252 = 15 * 16 + 12), 21 the longest prompt,
# 5 the shortest, 23 the last read of case B's 24; grids 0 (0, 15, 21, 117), 1 (16), 2 (5, 23, 251)
ORACLE_QWEN = (0, 5, 15, 16, 21, 23, 117, 251)
QWEN_LONGEST, QWEN_SHORTEST = 21, 5
# PaliGemma reads: page r % 12.  0 / 15 / 16 as above, 125 the last read of the 126-read call (chunk 7 of 8, partial) and in the
# middle chunk of the 252-read call, 251 its last read, 40 the longest prompt, 77 the shortest
ORACLE_PALI = (0, 15, 16, 40, 77, 125, 251)
PALI_LONGEST, PALI_SHORTEST = 40, 77
# top-1 on decisive steps (oracle margin > 0.05): at these random-init weights the logits sit at |x| ~ 4-8, where a bf16 ulp is 1/32
# and most margins are 2-5 ulps, so the suite's 6e-2 x scale bound admits an engine top-1 that differs from the oracle's.  Such a
# step is accepted only when the oracle itself holds the engine's choice within FLIP_ULPS bf16 ulps of its top-1, and at most
# MAX_FLIPS times per read (tests/_parity.check_logits)
FLIP_ULPS, MAX_FLIPS = 2, 2
REPORT = []


def _report(case, r, stats):
    REPORT.append((case, r, stats))
    print(f"[bench-geometry parity] {case} read {r}: mean {stats['mean']:.2e} p99.9 {stats['p999']:.2e} max {stats['max']:.2e} "
          f"(x scale; bounds 5e-3 / 3e-2 / 6e-2), decisive steps {stats['decisive']}, explained top-1 flips {len(stats['flips'])}")
    for f in stats["flips"]:
        print(f"[bench-geometry parity]   {f}")


def _general_layer(cfg, reads, fp8_kv, kind, splits):
    """The decode step of `cfg` at `reads` reads runs the general layer (no gemm_rows16 launch, the layer's GEMMs gemm_stream) and
    the attention instance `kind` with `splits` context splits (+ a merge when splits > 1).  Returns the plan."""
    from handwritten_ocr_amd import engine

    assert engine.pick_attn_splits(reads, cfg.kv_heads) == splits
    plan = engine.decode_plan(cfg, reads, fp8_kv=fp8_kv)
    assert not any("rows16" in l for l in plan["launches"]), plan["launches"]
    for g in engine.DECODE_GEMMS[:-1]:   # the layer's GEMMs (the LM head is gemm_skinny below 252 reads, gemm_stream256 at 252)
        assert plan[g][4].startswith("gemm_stream"), (g, plan[g])
    line = next(l for l in plan["launches"] if l.startswith("attn_decode_kernel"))
    assert plan["attn"].startswith(kind), plan["attn"]
    assert f"Hq={cfg.q_heads} Hkv={cfg.kv_heads} nsplit={splits} " in line, line
    if splits > 1:
        assert "+lastwg" in plan["attn"] or any("merge" in l for l in plan["launches"]), plan["launches"]
    return plan


def _engine(cfg, sd, ctx, fp8_kv):
    from handwritten_ocr_amd import engine

    eng = engine.ReadEngine(cfg, sd, ctx=ctx, fp8_kv=fp8_kv, **BENCH)
    assert eng.attn_splits == 0 and eng.fp8_kv == fp8_kv and not eng.fp8   # the splits decode_plan assumes; bf16 weights
    return eng


def _oracle_steps(step, last, cache, forced, eos):
    """The oracle's teacher-forced decode from the prompt's last logits: N_NEW steps of logits, top-1 with EOS suppressed."""
    steps, toks = [], []
    for n in range(N_NEW):
        lf = last.float().clone()
        lf[list(eos)] = -float("inf")
        steps.append(last)
        toks.append(int(torch.argmax(lf)))
        if n + 1 < N_NEW:
            last = step(int(forced[n]), cache)
    return torch.stack(steps), toks


def _engine_read(eng, pages, prompts, forced, reads):
    """generate(...) teacher-forced with logits; the oracle reads' logits indexed on the device before they come to the host."""
    t0 = time.perf_counter()
    toks, logits = eng.generate(pages, prompts, max_new=N_NEW, min_new=N_NEW, forced=forced, return_logits=True)
    out = {r: (logits[r].cpu(), toks[r]) for r in reads if r < len(pages)}
    del logits
    torch.cuda.empty_cache()
    print(f"[bench-geometry parity] engine call of {len(pages)} reads: {time.perf_counter() - t0:.1f} s")
    return out


def _check(case, got, want):
    for r, (lg, toks) in got.items():
        w, wt = want[r]
        _report(case, r, check_logits(lg, w, toks, wt, f"{case} read {r}", flip_ulps=FLIP_ULPS, max_flips=MAX_FLIPS))


# ------------------------------------------------------------------------------------------------------------------------------ Qwen
QWEN_SHAPES = ((1024, 1024), (1024, 704), (364, 532))   # raw page sizes -> 1008 x 1008, 1036 x 700 (portrait), 364 x 532 (landscape)


def _qwen_inputs(cfg):
    from handwritten_ocr_amd import imageproc, preprocess, synth, tokenizer
    from handwritten_ocr_amd.compat import config

    strategies = config.PREPROCESSING_STRATEGIES
    raw = {}   # (grid, i) -> strategy-applied PIL image; 12 distinct pages per grid
    for g, (h, w) in enumerate(QWEN_SHAPES):
        for i in range(12):
            raw[g, i] = preprocess.apply_strategy(Image.fromarray(synth.make_page(100 * g + i, h, w), "RGB"),
                                                  strategies[i % len(strategies)], quiet=True)
    arr = {k: imageproc.prepare_page(im, cfg.patch_size, cfg.merge, config.OCR_MIN_PIXELS, config.OCR_MAX_PIXELS) for k, im in raw.items()}
    shapes = sorted({a.shape for a in arr.values()})
    assert len(shapes) == 3 and any(s[0] > s[1] for s in shapes) and any(s[0] < s[1] for s in shapes), shapes
    proc = tokenizer.Processor(cfg, tokenizer.ByteTokenizer(cfg, fold_unknown=True))
    key = [(r % 3, (r // 3) % 12) for r in range(252)]
    pages = [arr[k] for k in key]
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz .,", np.uint8)
    rng = np.random.default_rng(1)

    def prompt(r, tail):
        text = config.OCR_PROMPT + " " + bytes(rng.choice(letters, size=tail)).decode() if tail else config.OCR_PROMPT
        return proc.chat_ids(text, proc.image_tokens(pages[r]))

    prompts = [prompt(r, 0 if r == QWEN_SHORTEST else (r * 37) % 300 + 1) for r in range(252)]
    # the longest: its padded prompt + N_NEW generated tokens fill the 2048-position cache (Tp = 1920, 57 positions left after the
    # last step)
    base = len(prompts[QWEN_LONGEST]) - ((QWEN_LONGEST * 37) % 300 + 1) - 1
    prompts[QWEN_LONGEST] = prompt(QWEN_LONGEST, 1920 - base - 1)
    T = [len(p) for p in prompts]
    assert T[QWEN_LONGEST] == 1920 == max(T) and T[QWEN_SHORTEST] == min(T) < 400, (max(T), min(T))
    for s0 in range(0, 252, 16):
        assert len(set(T[s0: s0 + 16])) == len(T[s0: s0 + 16]), "prompt lengths repeat inside a prefill chunk"
    forced = np.random.default_rng(2).integers(0, min(list(cfg.eos_ids) + [cfg.pad_id, cfg.image_token_id, cfg.vision_start_id]),
                                                size=(252, N_NEW)).astype(np.int32)
    return raw, key, pages, prompts, forced


def _qwen_ref_cfg(cfg):
    from oracle.qwen2vl_ref import RefConfig

    return RefConfig(depth=cfg.depth, embed_dim=cfg.embed_dim, num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, family=cfg.family,
                     vit_inter=cfg.vit_inter, window_size=cfg.window_size, fullatt=tuple(cfg.fullatt), hidden=cfg.hidden,
                     layers=cfg.layers, q_heads=cfg.q_heads, kv_heads=cfg.kv_heads, inter=cfg.inter, vocab=cfg.vocab, tie=cfg.tie,
                     image_token_id=cfg.image_token_id, vision_start_id=cfg.vision_start_id, vision_end_id=cfg.vision_end_id,
                     eos_ids=tuple(cfg.eos_ids), pad_id=cfg.pad_id)


def _qwen_oracle(cfg, sd_cpu, raw, key, prompts, forced, reads, kv_quant):
    """{read: (logits [N_NEW][V], top-1 tokens)} of the oracle with a bf16 cache, and (kv_quant) the same reads over the E4M3 cache:
    the prompt pass is shared (it attends over bf16 K / V either way; tests/test_oracle_kv_quant.py pins that the hooked oracle's
    cache after it is the round trip of this one's)."""
    from handwritten_ocr_amd.compat import config
    from oracle import image_ref
    from oracle.qwen2vl_ref import Qwen2VLRef, kv_round_trip, rope_index

    rc = _qwen_ref_cfg(cfg)
    ref, ref8 = Qwen2VLRef(rc, sd_cpu), Qwen2VLRef(rc, sd_cpu, kv_quant=True)
    embed = ref.w("model.language_model.embed_tokens.weight")
    tower = {}
    want, want8 = {}, {}
    t0 = time.perf_counter()
    with torch.no_grad():
        for r in reads:
            if key[r] not in tower:   # the tower once per distinct page
                pv, grid = image_ref.pixel_values(raw[key[r]], config.OCR_MIN_PIXELS, config.OCR_MAX_PIXELS)
                tower[key[r]] = (ref.vision(torch.from_numpy(pv), [grid]), grid)
            img, grid = tower[key[r]]
            ids = torch.from_numpy(np.asarray(prompts[r])).long()
            x = F.embedding(ids, embed).clone()
            x[ids == cfg.image_token_id] = img.to(x.dtype)
            pos3, delta = rope_index(ids, cfg.image_token_id, [grid], cfg.merge)
            cache = [None] * cfg.layers
            last = ref.lm_head(ref.decoder(x, pos3, cache)[-1:])[0]
            cache8 = [(kv_round_trip(k), kv_round_trip(v)) for k, v in cache] if kv_quant else None
            want[r] = _oracle_steps(lambda t, c: ref.step(t, c, delta), last, cache, forced[r], cfg.eos_ids)
            if kv_quant:
                want8[r] = _oracle_steps(lambda t, c: ref8.step(t, c, delta), last, cache8, forced[r], cfg.eos_ids)
    print(f"[bench-geometry parity] {cfg.name} oracle, {len(reads)} reads ({len(tower)} pages): {time.perf_counter() - t0:.1f} s")
    return want, want8


def _qwen_setup(preset, over, kv_quant):
    from handwritten_ocr_amd import engine

    cfg = dataclasses.replace(engine.preset(preset), depth=2, layers=2, **over)
    sd = engine.random_state_dict(cfg, seed=0, device="cuda")
    sd_cpu = {k: v.cpu() for k, v in engine.normalize_keys(sd).items()}
    raw, key, pages, prompts, forced = _qwen_inputs(cfg)
    want, want8 = _qwen_oracle(cfg, sd_cpu, raw, key, prompts, forced, ORACLE_QWEN, kv_quant)
    del sd_cpu
    return dict(cfg=cfg, sd=sd, pages=pages, prompts=prompts, forced=forced, want=want, want8=want8)


class TestQwen2VL2B:
    @pytest.fixture(scope="class")
    def q2b(self):
        d = _qwen_setup("qwen2-vl-2b", {}, kv_quant=True)
        d["eng"] = _engine(d["cfg"], d["sd"], 2048, fp8_kv=False)
        yield d
        d["eng"].close()

    def test_a_252_reads_general_layer_one_pass(self, q2b):
        from handwritten_ocr_amd import engine

        plan = _general_layer(q2b["cfg"], 252, False, "attn_decode_kernel<tiled,8,128>", 1)
        assert plan == engine.decode_plan(engine.preset("qwen2-vl-2b"), 252)   # the very instances the bench's decode step runs
        got = _engine_read(q2b["eng"], q2b["pages"], q2b["prompts"], q2b["forced"], ORACLE_QWEN)
        _check("A qwen2-vl-2b 252", got, q2b["want"])

    def test_b_24_reads_general_layer_split_attention(self, q2b):
        _general_layer(q2b["cfg"], 24, False, "attn_decode_kernel<tiled,4,128>", 16)
        got = _engine_read(q2b["eng"], q2b["pages"][:24], q2b["prompts"][:24], q2b["forced"][:24], ORACLE_QWEN)
        assert sorted(got) == [0, 5, 15, 16, 21, 23]
        _check("B qwen2-vl-2b 24", got, q2b["want"])

    def test_graph_replay_equals_eager_at_252_reads(self, q2b):
        eng = q2b["eng"]
        n_graphs = len(eng._graphs)
        eager = eng.generate(q2b["pages"], q2b["prompts"], max_new=N_NEW, use_graph=False)
        graph = eng.generate(q2b["pages"], q2b["prompts"], max_new=N_NEW, use_graph=True)
        assert len(eng._graphs) == n_graphs + 1, "the 252-read decode was not captured"
        again = eng.generate(q2b["pages"], q2b["prompts"], max_new=N_NEW, use_graph=True)   # a replay of the captured graph
        diff = [r for r in range(252) if graph[r] != eager[r]]
        assert not diff, f"graph replay differs from eager decode at reads {diff[:8]} (of {len(diff)})"
        assert again == eager
        assert sum(len(t) for t in eager) > 252 * 8, "too few generated tokens to compare"

    def test_a_252_reads_e4m3_cache(self, q2b):
        cfg = q2b["cfg"]
        _general_layer(cfg, 252, True, "attn_decode_kernel<e4m3,8,128>", 1)
        eng = _engine(cfg, q2b["sd"], 2048, fp8_kv=True)
        try:
            got = _engine_read(eng, q2b["pages"], q2b["prompts"], q2b["forced"], ORACLE_QWEN)
        finally:
            eng.close()
        _check("A e4m3 qwen2-vl-2b 252", got, q2b["want8"])


def test_c_qwen25_7b_252_reads_general_layer():
    d = _qwen_setup("qwen2.5-vl-7b", {"fullatt": (1,)}, kv_quant=False)
    cfg = d["cfg"]
    assert (cfg.q_heads, cfg.kv_heads) == (28, 4)
    _general_layer(cfg, 252, False, "attn_decode_kernel<tiled,8,128>", 1)
    eng = _engine(cfg, d["sd"], 2048, fp8_kv=False)
    try:
        got = _engine_read(eng, d["pages"], d["prompts"], d["forced"], ORACLE_QWEN)
    finally:
        eng.close()
    _check("C qwen2.5-vl-7b 252", got, d["want"])


# ------------------------------------------------------------------------------------------------------------------------ PaliGemma
def _pali_inputs(cfg):
    from handwritten_ocr_amd import imageproc, preprocess, synth
    from handwritten_ocr_amd.compat import config

    strategies = config.PREPROCESSING_STRATEGIES
    distinct = [imageproc.prepare_square(preprocess.apply_strategy(Image.fromarray(synth.make_page(300 + i, 1024, 1024), "RGB"),
                                                                   strategies[i % len(strategies)], quiet=True), cfg.image_size)
                for i in range(12)]
    pages = [distinct[r % 12] for r in range(252)]
    n_img = (cfg.image_size // cfg.patch_size) ** 2
    rng = np.random.default_rng(3)
    # text tails of 0..127 ids: distinct inside every prefill chunk; the longest fills Tp = 4224 (+ N_NEW = 4296 of 4352 positions)
    tails = [(r * 37) % 120 + 1 for r in range(252)]
    tails[PALI_LONGEST], tails[PALI_SHORTEST] = 4224 - n_img - 1, 0
    prompts = [np.asarray([cfg.image_token_id] * n_img + [cfg.bos_id] + rng.integers(3, 1000, size=t).tolist(), np.int32) for t in tails]
    T = [len(p) for p in prompts]
    assert T[PALI_LONGEST] == 4224 == max(T) and T[PALI_SHORTEST] == n_img + 1 == min(T)
    for s0 in range(0, 252, 16):
        assert len(set(T[s0: s0 + 16])) == len(T[s0: s0 + 16]), "prompt lengths repeat inside a prefill chunk"
    forced = np.random.default_rng(4).integers(3, 256000, size=(252, N_NEW)).astype(np.int32)
    return distinct, pages, prompts, forced


def _pali_oracle(cfg, sd_cpu, distinct, prompts, forced, reads):
    from oracle.paligemma_ref import PaliGemmaRef, PaliRefConfig
    from oracle.qwen2vl_ref import kv_round_trip
    from handwritten_ocr_amd import imageproc

    rc = PaliRefConfig(v_layers=cfg.depth, v_hidden=cfg.embed_dim, v_heads=cfg.num_heads, v_inter=cfg.vit_inter, patch_size=cfg.patch_size,
                       image_size=cfg.image_size, hidden=cfg.hidden, layers=cfg.layers, q_heads=cfg.q_heads, kv_heads=cfg.kv_heads,
                       head_dim=cfg.head_dim, inter=cfg.inter, vocab=cfg.vocab, rope_theta=cfg.rope_theta,
                       image_token_id=cfg.image_token_id, eos_ids=tuple(cfg.eos_ids), pad_id=cfg.pad_id)
    ref, ref8 = PaliGemmaRef(rc, sd_cpu), PaliGemmaRef(rc, sd_cpu, kv_quant=True)
    lut = imageproc.pixel_lut((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    tower, want, want8 = {}, {}, {}
    t0 = time.perf_counter()
    with torch.no_grad():
        for r in reads:
            i = r % 12
            if i not in tower:
                page = distinct[i]
                tower[i] = ref.vision(torch.from_numpy(np.stack([lut[c][page[:, :, c]] for c in range(3)])))
            ids = torch.from_numpy(prompts[r]).long()
            mask = ids == cfg.image_token_id
            x = ref.embed(torch.where(mask, torch.zeros_like(ids), ids))
            x[mask] = tower[i].to(x.dtype)
            cache = [None] * cfg.layers
            last = ref.lm_head(ref.decoder(x, torch.arange(len(ids)) + 1, cache, bidirectional=True)[-1:])[0]
            cache8 = [(kv_round_trip(k), kv_round_trip(v)) for k, v in cache]
            want[r] = _oracle_steps(ref.step, last, cache, forced[r], cfg.eos_ids)
            want8[r] = _oracle_steps(ref8.step, last, cache8, forced[r], cfg.eos_ids)
    print(f"[bench-geometry parity] {cfg.name} oracle, {len(reads)} reads ({len(tower)} pages): {time.perf_counter() - t0:.1f} s")
    return want, want8


class TestPaliGemma3B:
    @pytest.fixture(scope="class")
    def pg(self):
        from handwritten_ocr_amd import engine

        cfg = dataclasses.replace(engine.preset("paligemma-3b"), depth=2, layers=2)
        sd = engine.random_state_dict(cfg, seed=0, device="cuda")
        sd_cpu = {k: v.cpu() for k, v in engine.normalize_keys(sd).items()}
        distinct, pages, prompts, forced = _pali_inputs(cfg)
        want, want8 = _pali_oracle(cfg, sd_cpu, distinct, prompts, forced, ORACLE_PALI)
        del sd_cpu
        yield dict(cfg=cfg, sd=sd, pages=pages, prompts=prompts, forced=forced, want=want, want8=want8)

    @pytest.mark.parametrize("fp8_kv", [False, True], ids=["bf16_cache", "e4m3_cache"])
    def test_d_126_then_252_reads(self, pg, fp8_kv):
        cfg = pg["cfg"]
        kind = "attn_decode_kernel<e4m3,4,256>" if fp8_kv else "attn_decode_kernel<rows,4,256>"
        _general_layer(cfg, 126, fp8_kv, kind, 6)   # the ATTN_DECODE_BENCH_CASES pair: 6 splits + merge, then one pass
        _general_layer(cfg, 252, fp8_kv, kind, 1)
        want = pg["want8"] if fp8_kv else pg["want"]
        eng = _engine(cfg, pg["sd"], 4352, fp8_kv=fp8_kv)
        try:
            got = _engine_read(eng, pg["pages"][:126], pg["prompts"][:126], pg["forced"][:126], ORACLE_PALI)
            assert sorted(got) == [0, 15, 16, 40, 77, 125]
            _check(f"D{' e4m3' if fp8_kv else ''} paligemma-3b 126", got, want)
            got = _engine_read(eng, pg["pages"], pg["prompts"], pg["forced"], ORACLE_PALI)
            _check(f"D{' e4m3' if fp8_kv else ''} paligemma-3b 252", got, want)
        finally:
            eng.close()
