"""Loading helpers for tests/golden (data only: inputs + expected outputs written by tools/make_goldens.py)."""
import json
import os

import torch
from safetensors.torch import load_file

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_json(name):
    with open(os.path.join(GOLD, name), "r", encoding="utf-8") as f:
        return json.load(f)


STEM = {"qwen2_vl": "qwen2vl_tiny", "qwen2_5_vl": "qwen25vl_tiny"}
FAMILIES = tuple(STEM)


def tiny_meta(family="qwen2_vl"):
    return load_json(STEM[family] + ".json")


def tiny_weights(dtype=torch.bfloat16, family="qwen2_vl"):
    sd = load_file(os.path.join(GOLD, STEM[family] + "_weights.safetensors"))
    return {k: v.to(dtype) for k, v in sd.items()}


def tiny_case(tag, family="qwen2_vl"):
    return load_file(os.path.join(GOLD, f"{STEM[family]}_{tag}.safetensors"))


def tiny_ref_config(family="qwen2_vl"):
    from oracle.qwen2vl_ref import RefConfig

    m = tiny_meta(family)["config"]
    v, t = m["vision"], m["text"]
    if family == "qwen2_vl":
        tower = dict(embed_dim=v["embed_dim"], mlp_ratio=v["mlp_ratio"])
    else:
        tower = dict(embed_dim=v["hidden_size"], family=family, vit_inter=v["intermediate_size"],
                     window_size=v["window_size"], fullatt=tuple(v["fullatt_block_indexes"]))
    return RefConfig(depth=v["depth"], num_heads=v["num_heads"], patch_size=v["patch_size"], merge=v["spatial_merge_size"],
                     tps=v["temporal_patch_size"], hidden=t["hidden_size"], layers=t["num_hidden_layers"],
                     q_heads=t["num_attention_heads"], kv_heads=t["num_key_value_heads"], inter=t["intermediate_size"],
                     vocab=t["vocab_size"], rope_theta=t["rope_parameters"]["rope_theta"],
                     mrope_section=tuple(t["rope_parameters"]["mrope_section"]), eps=t["rms_norm_eps"],
                     image_token_id=m["image_token_id"], vision_start_id=m["vision_start_token_id"],
                     vision_end_id=m["vision_end_token_id"], tie=True, eos_ids=(m["eos"],), pad_id=m["pad"], **tower)


_HF_CASES = {}


def tiny_hf_case(family, case, dtype=torch.bfloat16):
    """The tensors of tiny_case() for one case, recomputed by the HF model itself on THIS host from the stored config, weights
    and inputs, loaded and run as tools/make_goldens.py does.  A bf16 golden holds the bits of the CPU that wrote it: oneDNN
    sums a bf16 GEMM in another order with AMX than with AVX-512 / AVX2, and the rounding flips grow through the layers (up to
    ~3 bf16 ulps of the logits' scale), while the oracle and HF agree bit for bit on any one host."""
    key = (family, case, dtype)
    if key in _HF_CASES:
        return _HF_CASES[key]
    import tempfile

    if family == "qwen2_vl":
        from transformers import Qwen2VLConfig as Cfg, Qwen2VLForConditionalGeneration as Model
    else:
        from transformers import Qwen2_5_VLConfig as Cfg, Qwen2_5_VLForConditionalGeneration as Model
    meta = tiny_meta(family)
    spec, cm = meta["config"], meta["cases"][case]
    cfg = Cfg(vision_config=dict(spec["vision"]), text_config=dict(spec["text"]), image_token_id=spec["image_token_id"],
              video_token_id=spec["video_token_id"], vision_start_token_id=spec["vision_start_token_id"],
              vision_end_token_id=spec["vision_end_token_id"], tie_word_embeddings=True)
    model = Model(cfg).eval()
    missing, unexpected = model.load_state_dict(tiny_weights(torch.float32, family), strict=False)
    assert missing == ["lm_head.weight"] and not unexpected, (missing, unexpected)
    model.tie_weights()
    with tempfile.TemporaryDirectory() as tmp:  # from_pretrained(dtype=bf16): parameters bf16, rotary inv_freq buffers fp32
        model.save_pretrained(tmp)
        model = Model.from_pretrained(tmp, dtype=dtype).eval()
    model.generation_config.eos_token_id = spec["eos"]
    model.generation_config.pad_token_id = spec["pad"]
    g = tiny_case("fp32" if dtype == torch.float32 else "bf16", family)
    ids = g[f"{case}.input_ids"].long()[None]
    args = dict(input_ids=ids, pixel_values=g[f"{case}.pixel_values"], image_grid_thw=torch.tensor([cm["grid_thw"]]),
                mm_token_type_ids=(ids == spec["image_token_id"]).int(), attention_mask=torch.ones_like(ids))
    acts = {}

    def hook(name):
        def fn(mod, inp, outp):
            acts[name] = (outp[0] if isinstance(outp, tuple) else outp).detach().clone()
        return fn

    vis = model.model.visual
    hs = [vis.patch_embed.register_forward_hook(hook("patch_embed")), vis.blocks[0].register_forward_hook(hook("vit_block0")),
          vis.blocks[-1].register_forward_hook(hook("vit_last")),
          vis.register_forward_hook(lambda m_, i_, o_: acts.__setitem__("merger", o_.pooler_output.detach().clone())),
          model.model.language_model.layers[0].register_forward_hook(hook("dec_layer0"))]
    with torch.no_grad():
        fw = model(**args)
    for h in hs:
        h.remove()
    n = cm["n_new"]
    with torch.no_grad():
        rp = model.generate(**args, do_sample=False, max_new_tokens=n, min_new_tokens=n, repetition_penalty=cm["repetition_penalty"],
                            output_scores=True, return_dict_in_generate=True)
    out = {f"{case}.{k}": (v[0] if v.dim() == 3 else v) for k, v in acts.items()}
    out[f"{case}.prefill_logits"] = fw.logits[0]
    out[f"{case}.rp_tokens"] = rp.sequences[0, ids.shape[1]:].to(torch.int32)
    out[f"{case}.rp_scores"] = torch.stack([sc[0] for sc in rp.scores]).float()
    _HF_CASES[key] = out
    return out


# ------------------------------------------------------------------------------------------------ trained tiny checkpoints
TRAINED = {"qwen2_vl": "trained_qwen2vl", "qwen2_5_vl": "trained_qwen25vl", "paligemma": "trained_paligemma"}
TRAINED_FAMILIES = tuple(TRAINED)


def trained_meta(family="qwen2_vl"):
    """tests/golden/trained_*.json: HF's own transcriptions (token streams + decoded text) of 8 synthetic pages by the briefly
    trained tiny checkpoint in tests/golden/trained_*/ (tools/make_goldens.py --only trained,trained25)."""
    return load_json(TRAINED[family] + ".json")


def trained_dir(family="qwen2_vl"):
    return os.path.join(GOLD, TRAINED[family])


def trained_page(case):
    """The page a fixture case was transcribed from (regenerated: synth.make_page + its paper colour)."""
    from handwritten_ocr_amd.synth import make_page, tint_page

    return tint_page(make_page(case["page_seed"], *case["page_hw"]), case["page_tint"])


def mean_cer(want_texts, got_texts):
    """The reference's metric over a set of pages: cer() per page (ocr_agent/tools.py:103-118, restated bit-exactly in
    handwritten_ocr_amd.text and pinned by text_kats.json), averaged."""
    from handwritten_ocr_amd import text

    return sum(text.cer(w, g) for w, g in zip(want_texts, got_texts)) / len(want_texts)
