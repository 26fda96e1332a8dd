"""Which KV cache an engine keeps (engine.kv_cache_e4m3): the request ReadEngine(fp8_kv=...) x the weight precision x the head width x
the environment (HWOCR_FP8_KV, HWOCR_KV_DTYPE).  Host-only: the rule is a pure function, no device needed."""
import itertools

import pytest

from handwritten_ocr_amd import engine


def _before(fp8_kv, fp8, head_dim, env):
    """The rule as it stood before the 128-wide E4M3 cache: only the fp8 engine of a 256-wide-head model, on by default."""
    return fp8 and head_dim == 256 and (env.get("HWOCR_FP8_KV", "1") not in ("", "0") if fp8_kv is None else bool(fp8_kv))


ENVS = [{}, {"HWOCR_FP8_KV": "0"}, {"HWOCR_FP8_KV": "1"}, {"HWOCR_FP8_KV": ""}]


@pytest.mark.parametrize("fp8,head_dim,env", list(itertools.product([False, True], [128, 256], ENVS)))
def test_the_default_is_todays_rule_exactly(fp8, head_dim, env):
    assert engine.kv_cache_e4m3(None, fp8, head_dim, env) == _before(None, fp8, head_dim, env)


@pytest.mark.parametrize("fp8,head_dim,env", list(itertools.product([False, True], [128, 256], ENVS + [{"HWOCR_KV_DTYPE": "e4m3"},
                                                                                                        {"HWOCR_KV_DTYPE": "bf16"}])))
def test_an_explicit_request_wins_over_weights_width_and_environment(fp8, head_dim, env):
    assert engine.kv_cache_e4m3(True, fp8, head_dim, env) is True
    assert engine.kv_cache_e4m3(False, fp8, head_dim, env) is False


def test_the_only_change_is_fp8_kv_true_without_fp8_or_at_128():
    for fp8_kv, fp8, hd, env in itertools.product([None, True, False], [False, True], [128, 256], ENVS):
        new, old = engine.kv_cache_e4m3(fp8_kv, fp8, hd, env), _before(fp8_kv, fp8, hd, env)
        if new != old:
            assert fp8_kv is True and (not fp8 or hd == 128) and new and not old


@pytest.mark.parametrize("fp8,head_dim", list(itertools.product([False, True], [128, 256])))
def test_hwocr_kv_dtype_decides_when_nothing_is_requested(fp8, head_dim):
    for v in ("e4m3", "E4M3", " e4m3 "):
        assert engine.kv_cache_e4m3(None, fp8, head_dim, {"HWOCR_KV_DTYPE": v}) is True
        assert engine.kv_cache_e4m3(None, fp8, head_dim, {"HWOCR_KV_DTYPE": v, "HWOCR_FP8_KV": "0"}) is True
    assert engine.kv_cache_e4m3(None, fp8, head_dim, {"HWOCR_KV_DTYPE": "bf16"}) is False
    assert engine.kv_cache_e4m3(None, fp8, head_dim, {"HWOCR_KV_DTYPE": ""}) == _before(None, fp8, head_dim, {})


def test_unknown_values_and_widths_are_refused():
    with pytest.raises(ValueError):
        engine.kv_cache_e4m3(None, False, 128, {"HWOCR_KV_DTYPE": "fp8"})
    with pytest.raises(ValueError):
        engine.kv_cache_e4m3(True, False, 64, {})


def test_the_process_environment_is_read_when_none_is_given(monkeypatch):
    monkeypatch.setenv("HWOCR_KV_DTYPE", "e4m3")
    assert engine.kv_cache_e4m3(None, False, 128) is True
    monkeypatch.delenv("HWOCR_KV_DTYPE")
    monkeypatch.delenv("HWOCR_FP8_KV", raising=False)
    assert engine.kv_cache_e4m3(None, False, 128) is False and engine.kv_cache_e4m3(None, True, 256) is True


def test_the_launch_plans_list_the_e4m3_instances_at_128():
    """Plan recording (no device): a Qwen2-VL-2B decode step with an E4M3 cache runs the KV8 attention instance at 128, the 8-wave form
    at 252 reads and the 4-wave split form at 3; its prefill fills the cache with the 128-wide quantiser."""
    cfg = engine.preset("qwen2-vl-2b")
    assert "e4m3" not in engine.decode_plan(cfg, 252)["attn"]
    a252, a3 = engine.decode_plan(cfg, 252, fp8_kv=True)["attn"], engine.decode_plan(cfg, 3, fp8_kv=True)["attn"]
    assert a252.startswith("attn_decode_kernel<e4m3,8,128>"), a252
    assert a3.startswith("attn_decode_kernel<e4m3,4,128>"), a3
    lines = engine.wide_plan(cfg, (1008, 1008), 2, 2, 1328, False, fp8_kv=True)
    assert sum(l.startswith("kv_quant_fp8_kernel<128>") for l in lines) == cfg.layers
