"""Teacher-forced logits of the engine against the CPU oracle: the suite's full-width tolerance (tests/test_model_gpu.py, SURVEY.md
8c), shared by tests/test_fullwidth_oracle_gpu.py and tests/test_bench_geometry_oracle_gpu.py.

Mean-abs error <= 5e-3 x scale, 99.9 % of the logits within 3e-2 x scale, none beyond 6e-2 x scale (scale = max(1, max |logit|)),
and top-1 agreement on every step whose oracle margin exceeds 0.05."""
import torch


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """The bf16 spacing at |x| (normal range): 2^(floor(log2 |x|) - 7)."""
    return torch.exp2(torch.floor(torch.log2(x.abs().float().clamp_min(2.0 ** -126))) - 7)


def quantile(x: torch.Tensor, q: float) -> float:
    """torch.quantile(x, q) (linear interpolation) of a flat tensor, also past its 2^24-element limit (72 steps x 257 216 logits)."""
    if x.numel() < 2 ** 24:
        return float(x.quantile(q))
    pos = q * (x.numel() - 1)
    lo = int(pos)
    a = float(x.kthvalue(lo + 1).values)
    b = float(x.kthvalue(min(lo + 2, x.numel())).values)
    return a + (pos - lo) * (b - a)


def check_logits(got, want, toks_engine, toks_oracle, what, flip_ulps=0, max_flips=0):
    """got / want [steps][V]; toks_*: the top-1 token of every step.  Returns the three error / scale ratios (for reports).

    flip_ulps > 0 (default 0: every decisive step must agree): a decisive step whose engine top-1 differs is accepted when the
    oracle's logit of the engine's choice lies within flip_ulps bf16 ulps of the oracle's top-1 logit, at most max_flips times."""
    got, want = got.float().cpu(), want.float()
    scale = max(1.0, float(want.abs().max()))
    d = (got - want).abs()
    mean, p999, mx = float(d.mean()), quantile(d.flatten(), 0.999), float(d.max())
    assert mean <= 5e-3 * scale, f"{what}: mean logit error {mean} (scale {scale})"
    assert p999 <= 3e-2 * scale, f"{what}: p99.9 {p999} (scale {scale})"
    assert mx <= 6e-2 * scale, f"{what}: teacher-forced logits differ by {mx} (scale {scale})"
    top2 = want.topk(2, -1).values
    decisive = (top2[:, 0] - top2[:, 1]) > 0.05
    agree = torch.tensor([a == b for a, b in zip(toks_engine, toks_oracle)])
    flips = []
    if flip_ulps:
        for s in torch.nonzero(decisive & ~agree).flatten().tolist():
            te, to = toks_engine[s], toks_oracle[s]
            gap = float(want[s, to] - want[s, te])
            ulp = float(bf16_ulp(want[s, to]))
            detail = (f"{what}: step {s} engine top-1 {te}, oracle {to}: oracle gap {gap} = {gap / ulp:.1f} bf16 ulps, errors "
                      f"{float(got[s, te] - want[s, te]):+.4f} / {float(got[s, to] - want[s, to]):+.4f}")
            assert gap <= flip_ulps * ulp, detail
            flips.append(detail)
        assert len(flips) <= max_flips, flips
        agree[decisive & ~agree] = True
    assert bool(agree[decisive].all()), (what, toks_engine, toks_oracle)
    return {"mean": mean / scale, "p999": p999 / scale, "max": mx / scale, "decisive": int(decisive.sum()), "flips": flips}
