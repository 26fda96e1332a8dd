"""CPU checks of the range tests' own helpers (tests/_ranges.py): the E4M3 code enumeration really holds every finite code and every
rounding tie, and the E4M3 KV error bound is never violated yet not vacuous."""
import math

import torch

from oracle import fp8_ref
from tests._ranges import (coverage_codes, e4m3_finite_codes, e4m3_grid, e4m3_quant_pool, e4m3_values, kv8_error_bound,
                           softmax_attention64)


def test_exactly_254_finite_codes():
    c = e4m3_finite_codes()
    assert c.numel() == 254 and len(set(c.tolist())) == 254
    assert 0x7F not in c.tolist() and 0xFF not in c.tolist()
    v = e4m3_values(c)
    assert bool(torch.isfinite(v).all())
    assert float(v.max()) == 448.0 and float(v.min()) == -448.0
    assert 0x00 in c.tolist() and 0x80 in c.tolist()                        # +0 and -0
    assert float(v[v > 0].min()) == 2.0 ** -9                                 # the smallest subnormal
    assert int(((c & 0x78) == 0).sum()) == 16                                 # exponent field 0: ±0 and 14 subnormals


def test_coverage_codes_hold_every_code_in_any_254_window():
    full = set(e4m3_finite_codes().tolist())
    cc = coverage_codes(1000, offset=5)
    for start in (0, 1, 100, 746):
        assert set(cc[start:start + 254].tolist()) == full


def test_quant_pool_is_every_code_and_every_midpoint_exact_in_bf16():
    mags, mids = e4m3_grid()
    assert mags.numel() == 127 and mids.numel() == 126
    assert bool((mids > mags[:-1]).all() and (mids < mags[1:]).all())
    pool = e4m3_quant_pool()
    assert pool.numel() == 2 * (127 + 126)
    assert torch.equal(pool.to(torch.bfloat16).float(), pool)                # the kernels' inputs are bf16: no rounding on the way in
    # scale 1 (row max 448): the codes themselves map to themselves; every midpoint goes to the neighbour with the even code
    q, s = fp8_ref.quant_rows(pool.view(1, -1))
    assert float(s) == 1.0
    qv = q.float().flatten()
    n = 127
    assert torch.equal(qv[:n], mags)
    lo, hi = torch.arange(126), torch.arange(1, 127)
    even = torch.where(lo % 2 == 0, mags[lo], mags[hi])
    assert torch.equal(qv[n:2 * n - 1], even)


def _perturbed(q, k, v, scale, eps, vmax, g):
    """A key / value perturbation inside the bound's premises: |scale q.(k' - k)| <= eps for every key, |v' - v| <= vmax."""
    dk = torch.randn(k.shape, generator=g, dtype=torch.float64)
    # scale each key's perturbation so that the largest |logit change| over the queries is eps * u, u in [0, 1]
    lg = (scale * (q @ dk.t())).abs().amax(dim=0)                              # [n]
    dk = dk * (eps * torch.rand(k.shape[0], generator=g, dtype=torch.float64) / lg.clamp_min(1e-300))[:, None]
    dv = (2 * torch.rand(v.shape, generator=g, dtype=torch.float64) - 1) * vmax
    return k + dk, v + dv


def test_kv8_bound_holds_against_brute_force_perturbations():
    g = torch.Generator().manual_seed(17)
    worst = 0.0
    for trial in range(200):
        n, d, hq = int(torch.randint(1, 40, (1,), generator=g)), 16, 3
        scale = d ** -0.5
        q = torch.randn(hq, d, generator=g, dtype=torch.float64) * (1 + 3 * (trial % 4))
        k = torch.randn(n, d, generator=g, dtype=torch.float64)
        v = torch.randn(n, d, generator=g, dtype=torch.float64) * 2
        eps, vmax = 10 ** float(torch.empty(1).uniform_(-4, 0.5, generator=g)), 10 ** float(torch.empty(1).uniform_(-4, -1, generator=g))
        k2, v2 = _perturbed(q, k, v, scale, eps, vmax, g)
        bound = kv8_error_bound(q, k, k2, v, v2, scale)
        o, _ = softmax_attention64(q, k, v, scale)
        o2, _ = softmax_attention64(q, k2, v2, scale)
        err = (o2 - o).abs()
        assert bool((err <= bound * (1 + 1e-12) + 1e-15).all()), f"trial {trial}: bound violated by {float((err - bound).max())}"
        worst = max(worst, float((err / bound).max()))
    assert worst > 0.05, worst


def test_kv8_bound_is_not_vacuous():
    """Two keys of equal logit with values +1 / -1; the keys move the logits by +eps / -eps: o' = tanh(eps), the bound 2 eps."""
    eps = 1e-2
    q = torch.tensor([[1.0, 0.0]], dtype=torch.float64)
    k = torch.zeros(2, 2, dtype=torch.float64)
    k2 = torch.tensor([[eps, 0.0], [-eps, 0.0]], dtype=torch.float64)
    v = torch.tensor([[1.0, 0.0], [-1.0, 0.0]], dtype=torch.float64)
    bound = kv8_error_bound(q, k, k2, v, v, 1.0)
    o, _ = softmax_attention64(q, k, v, 1.0)
    o2, _ = softmax_attention64(q, k2, v, 1.0)
    err = float((o2 - o).abs()[0, 0])
    assert abs(err - math.tanh(eps)) < 1e-12
    assert 0.05 < err / float(bound[0, 0]) <= 1.0
