"""The oracle's E4M3 KV cache hook (Qwen2VLRef / PaliGemmaRef kv_quant=True), which tests/test_bench_geometry_oracle_gpu.py compares
the engine's fp8_kv=True decode against.  It restates the cache contract of DESIGN.md §2 and include/hwocr.h (hwocr_kv.fp8):

  * off (the default), it changes nothing: the cache holds the bf16 rows HF's DynamicCache would;
  * on, the prompt still attends over bf16 K / V, and afterwards every cached (kv head, token) row is exactly the
    oracle/fp8_ref.quant_rows round trip of that bf16 row;
  * a decode step quantises the row it appends BEFORE it attends over it, as the fused decode kernel does."""
import torch
import torch.nn.functional as F

from oracle import fp8_ref
from oracle.paligemma_ref import PaliGemmaRef, PaliRefConfig
from oracle.qwen2vl_ref import Qwen2VLRef, RefConfig, kv_round_trip

QCFG = RefConfig(depth=1, embed_dim=64, num_heads=2, hidden=512, layers=2, q_heads=4, kv_heads=2, inter=96, vocab=300,
                 image_token_id=290, vision_start_id=291, vision_end_id=292, eos_ids=(299,), pad_id=298)
PCFG = PaliRefConfig(v_layers=1, v_hidden=64, v_heads=2, v_inter=96, patch_size=14, image_size=28, hidden=128, layers=2, q_heads=2,
                     kv_heads=1, head_dim=128, inter=96, vocab=300, image_token_id=300)


def _decoder_sd(prefix, cfg, bias, g):
    hd = cfg.head_dim
    sd = {prefix + "embed_tokens.weight": torch.randn(cfg.vocab, cfg.hidden, generator=g),
          prefix + "norm.weight": 1 + 0.1 * torch.randn(cfg.hidden, generator=g)}
    for l in range(cfg.layers):
        p = f"{prefix}layers.{l}."
        for n, rows in (("q", cfg.q_heads * hd), ("k", cfg.kv_heads * hd), ("v", cfg.kv_heads * hd)):
            sd[p + f"self_attn.{n}_proj.weight"] = 0.3 * torch.randn(rows, cfg.hidden, generator=g)
            if bias:
                sd[p + f"self_attn.{n}_proj.bias"] = torch.randn(rows, generator=g)
        sd[p + "self_attn.o_proj.weight"] = 0.1 * torch.randn(cfg.hidden, cfg.q_heads * hd, generator=g)
        sd[p + "mlp.gate_proj.weight"] = 0.1 * torch.randn(cfg.inter, cfg.hidden, generator=g)
        sd[p + "mlp.up_proj.weight"] = 0.1 * torch.randn(cfg.inter, cfg.hidden, generator=g)
        sd[p + "mlp.down_proj.weight"] = 0.1 * torch.randn(cfg.hidden, cfg.inter, generator=g)
        sd[p + "input_layernorm.weight"] = 1 + 0.1 * torch.randn(cfg.hidden, generator=g)
        sd[p + "post_attention_layernorm.weight"] = 1 + 0.1 * torch.randn(cfg.hidden, generator=g)
    return {k: v.to(torch.bfloat16) for k, v in sd.items()}


def _qwen_prompt(T=40):
    x = torch.randn(T, QCFG.hidden, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    pos3 = torch.arange(T).view(1, -1).expand(3, -1)
    return x, pos3


def _capture_attention(monkeypatch):
    """Every scaled_dot_product_attention call of the oracle: (q, k, v) as it was called."""
    calls = []
    real = F.scaled_dot_product_attention

    def spy(q, k, v, **kw):
        calls.append((q, k, v))
        return real(q, k, v, **kw)

    monkeypatch.setattr(F, "scaled_dot_product_attention", spy)
    return calls


def test_kv_round_trip_is_quant_rows_per_head_and_token():
    x = (torch.randn(3, 40, 128, generator=torch.Generator().manual_seed(1)) * torch.logspace(-3, 2, 40).view(1, -1, 1)).to(torch.bfloat16)
    x[1, 7] = 0   # an all-zero row: scale 1, codes 0
    got = kv_round_trip(x)
    assert got.dtype == torch.float32 and got.shape == x.shape
    for h in range(3):
        q, s = fp8_ref.quant_rows(x[h])
        assert torch.equal(got[h], q.float() * s[:, None])
    assert not torch.equal(got, x.float())   # it does round: E4M3 keeps 3 mantissa bits
    assert float(((got - x.float()).abs() / x.float().abs().amax(-1, keepdim=True).clamp_min(1e-30)).max()) <= 2 ** -4


def test_qwen_hook_off_is_the_identity_and_on_holds_the_round_trip(monkeypatch):
    sd = _decoder_sd("model.language_model.", QCFG, True, torch.Generator().manual_seed(0))
    off, on = Qwen2VLRef(QCFG, sd), Qwen2VLRef(QCFG, sd, kv_quant=True)
    assert not Qwen2VLRef(QCFG, sd).kv_quant
    x, pos3 = _qwen_prompt()
    c_off, c_on = [None] * QCFG.layers, [None] * QCFG.layers
    h_off = off.decoder(x, pos3, c_off)
    h_on = on.decoder(x, pos3, c_on)
    # the prompt attends over bf16 K / V either way; off, the cache holds them
    assert torch.equal(h_off, h_on)
    for l in range(QCFG.layers):
        assert c_off[l][0].dtype == torch.bfloat16 and c_off[l][0].shape == (QCFG.kv_heads, 40, QCFG.head_dim)
        # on: every cached row is exactly the quant_rows round trip of the bf16 row
        assert torch.equal(c_on[l][0], kv_round_trip(c_off[l][0])) and torch.equal(c_on[l][1], kv_round_trip(c_off[l][1]))
    # a decode step: the appended row is quantised BEFORE the step attends over it
    calls = _capture_attention(monkeypatch)
    lg_off = off.step(17, c_off, 0)
    assert all(k.dtype == torch.bfloat16 for _, k, _ in calls)
    calls.clear()
    lg_on = on.step(17, c_on, 0)
    g = QCFG.q_heads // QCFG.kv_heads
    for l in range(QCFG.layers):
        k_new, v_new = c_on[l][0][:, -1:], c_on[l][1][:, -1:]
        if l == 0:   # layer 0 sees the same input in both modes: its appended row is the round trip of the bf16-cache one
            assert torch.equal(k_new, kv_round_trip(c_off[0][0][:, -1:])) and torch.equal(v_new, kv_round_trip(c_off[0][1][:, -1:]))
        _, kk, vv = calls[l]
        assert kk.dtype == torch.float32 and kk.shape[2] == 41
        assert torch.equal(kk[0, :, -1:], k_new.repeat_interleave(g, dim=0)) and torch.equal(vv[0, :, -1:], v_new.repeat_interleave(g, dim=0))
        assert torch.equal(kk[0, :, :40], c_on[l][0][:, :40].repeat_interleave(g, dim=0))
    assert lg_on.dtype == lg_off.dtype and not torch.equal(lg_on, lg_off)


def test_qwen_hook_attends_in_fp32_over_the_dequantised_rows():
    """One decode step's attention output restated by hand: softmax(q k^T / sqrt(d)) v over the fp32 round-trip rows, rounded once."""
    from oracle.qwen2vl_ref import attend

    g = torch.Generator().manual_seed(5)
    q = torch.randn(4, 1, 128, generator=g).to(torch.bfloat16)
    k = kv_round_trip(torch.randn(4, 33, 128, generator=g).to(torch.bfloat16))
    v = kv_round_trip(torch.randn(4, 33, 128, generator=g).to(torch.bfloat16))
    got = attend(q, k, v, None, 128 ** -0.5)
    p = torch.softmax((q.double() @ k.double().transpose(1, 2)) * 128 ** -0.5, -1)
    want = (p @ v.double()).float()
    assert got.dtype == torch.bfloat16
    assert float((got.float() - want).abs().max()) <= 2 ** -8 * float(want.abs().max())
    # bf16 operands keep the plain bf16 call, bit for bit
    kb, vb = k.to(torch.bfloat16), v.to(torch.bfloat16)
    assert torch.equal(attend(q, kb, vb, None, 0.1), F.scaled_dot_product_attention(q[None], kb[None], vb[None], scale=0.1)[0])


def test_paligemma_hook_off_is_the_identity_and_on_holds_the_round_trip(monkeypatch):
    sd = _decoder_sd("model.language_model.", PCFG, False, torch.Generator().manual_seed(1))
    off, on = PaliGemmaRef(PCFG, sd), PaliGemmaRef(PCFG, sd, kv_quant=True)
    x = torch.randn(30, PCFG.hidden, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    pos = torch.arange(30) + 1
    c_off, c_on = [None] * PCFG.layers, [None] * PCFG.layers
    assert torch.equal(off.decoder(x, pos, c_off, bidirectional=True), on.decoder(x, pos, c_on, bidirectional=True))
    for l in range(PCFG.layers):
        assert c_off[l][0].dtype == torch.bfloat16
        assert torch.equal(c_on[l][0], kv_round_trip(c_off[l][0])) and torch.equal(c_on[l][1], kv_round_trip(c_off[l][1]))
    calls = _capture_attention(monkeypatch)
    lg_off = off.step(9, c_off)
    lg_on = on.step(9, c_on)
    assert torch.equal(c_on[0][0][:, -1:], kv_round_trip(c_off[0][0][:, -1:]))
    for l in range(PCFG.layers):
        _, kk, vv = calls[PCFG.layers + l]
        assert kk.dtype == torch.float32 and torch.equal(kk[0, :, -1:], c_on[l][0][:, -1:].repeat_interleave(PCFG.q_heads, dim=0))
        assert torch.equal(vv[0, :, -1:], c_on[l][1][:, -1:].repeat_interleave(PCFG.q_heads, dim=0))
    assert not torch.equal(lg_on, lg_off)
