"""Value generators and float64 references for the range tests (tests/test_ops_ranges_gpu.py): operands at the values real
checkpoints produce rather than N(0, 1) — dominant attention logits, pre-activations past the fp32 `exp` overflow, outlier channels,
every E4M3 code.  Host-only: importable without a GPU (tests/test_ranges_ref.py checks these helpers on the CPU)."""
import math

import torch

E4M3_MAX = 448.0


def e4m3_finite_codes() -> torch.Tensor:
    """The 254 finite E4M3 ("e4m3fn") codes as uint8: every byte but the two NaN patterns 0x7F / 0xFF (±0 both included)."""
    c = torch.arange(256, dtype=torch.int32)
    return c[(c & 0x7F) != 0x7F].to(torch.uint8)


def e4m3_values(codes: torch.Tensor) -> torch.Tensor:
    return codes.view(torch.float8_e4m3fn).float()


def e4m3_grid() -> tuple[torch.Tensor, torch.Tensor]:
    """(values, midpoints): the 127 non-negative finite E4M3 magnitudes 0 .. 448 ascending, and the 126 midpoints between
    neighbours (the round-to-nearest-even ties; every one of them is exact in bf16: 4 significant bits)."""
    mags = e4m3_values(torch.arange(0x7F, dtype=torch.uint8))
    return mags, 0.5 * (mags[1:] + mags[:-1])


def e4m3_quant_pool() -> torch.Tensor:
    """fp32 values that a scale-1 quantiser (row max 448) must map bit-exactly: every finite code, every midpoint between neighbouring
    codes, both signs, and ±448 — 506 values, all exact in bf16."""
    mags, mids = e4m3_grid()
    pos = torch.cat([mags, mids])
    return torch.cat([pos, -pos])


def coverage_codes(n: int, offset: int = 0) -> torch.Tensor:
    """n uint8 codes walking the 254 finite codes in a scrambled order: any 254 consecutive entries hold every code once
    (stride 97 is coprime with 254)."""
    codes = e4m3_finite_codes()
    return codes[(torch.arange(n) * 97 + offset) % 254]


def row_scales(n: int, lo: float, hi: float, g: torch.Generator) -> torch.Tensor:
    """n log-spaced magnitudes lo .. hi in a seeded random order."""
    s = torch.logspace(math.log10(lo), math.log10(hi), n)
    return s[torch.randperm(n, generator=g)]


def softmax_attention64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> tuple[torch.Tensor, torch.Tensor]:
    """float64 attention of queries q [..., Hq, d] over keys k / values v [..., n, d] shared by all of them (one kv head):
    (out [..., Hq, d], weights [..., Hq, n])."""
    s = (q.double() @ k.double().transpose(-1, -2)) * scale
    pw = torch.softmax(s, dim=-1)
    return pw @ v.double(), pw


def kv8_error_bound(q, k, kdeq, v, vdeq, scale):
    """Rigorous bound on |attn(q, kdeq, vdeq) - attn(q, k, v)| per output feature, float64.
    The logits move by d_j = scale q.(kdeq_j - k_j), |d_j| <= eps; the weights then move by a factor in [e^-2eps, e^2eps], so
    |p'_j - p_j| <= (e^{2 eps} - 1) p_j, and
        |o' - o| <= sum_j |p'_j - p_j| |v_j| + sum_j p'_j |v'_j - v_j| <= (e^{2 eps} - 1) sum_j p_j |v_j| + max_j |v'_j - v_j|.
    q [Hq, d]; k, kdeq, v, vdeq [n, d].  Returns [Hq, d]."""
    q, k, kdeq, v, vdeq = (t.double() for t in (q, k, kdeq, v, vdeq))
    eps = scale * (q @ (k - kdeq).t()).abs().amax(dim=-1, keepdim=True)          # [Hq, 1]
    _, pw = softmax_attention64(q, k, v, scale)
    return torch.expm1(2.0 * eps) * (pw @ v.abs()) + (vdeq - v).abs().amax(dim=0, keepdim=True)
