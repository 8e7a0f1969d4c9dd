"""CPU: the restatement of tests/quantile_refs.py against every output the reference produced for tests/golden/quantile_filter.npz (all 43
strategies at two quantiles; the dims, video, ties, single, pow_, nqfac_, list_ and zeroq_ families), at the tolerance the GPU test of the
same cases uses.  This is what entitles tests/test_gpu_quantile_edges.py to trust the restatement at shapes the reference cannot reach."""
import json

import numpy as np
import pytest
import torch

from tests import quantile_refs as R
from tests.conftest import GOLDEN

TRANSCENDENTAL = ("tanh", "sigmoid", "sin", "cos", "atan")


def _golden():
    g = np.load(f"{GOLDEN}/quantile_filter.npz", allow_pickle=False)
    return g, json.loads(str(g["meta_json"]))


CASES = sorted(k for k, v in _golden()[1].items() if "input" in v and v["error"] is None)


def test_the_golden_covers_every_strategy():
    meta = _golden()[1]
    names = {meta[k]["kwargs"].get("strategy", "clamp") for k in CASES}
    assert len(names) == 43 and len(CASES) > 200
    assert {k for k in names if k.startswith(("sin", "cos"))} == set(R.WAVES)


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference(name):
    g, meta = _golden()
    kw = dict(meta[name]["kwargs"])
    x = torch.from_numpy(g[f"in_{meta[name]['input']}"])
    want = torch.from_numpy(g[f"out_{name}"])
    strategy = kw.get("strategy", "clamp")
    pow_fac = kw.get("pow_fac", 0.5)
    got, stats = R.restate(x, kw.get("quantile", 0.75), kw.get("dim", 1), kw.get("flatten", True), strategy, pow_fac, kw.get("nq_fac", 1.0))
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(want.shape)
    rows = R._rows(x, kw.get("dim", 1), kw.get("flatten", True))[0].shape[0]
    assert all(tuple(s.shape) == (rows,) for s in stats)
    tol = 4e-6 if strategy.startswith(TRANSCENDENTAL) or pow_fac not in (0.0, 1.0, 0.5, 2.0) else 2e-6
    finite = torch.isfinite(want)
    peak = float(want[finite].abs().max()) if bool(finite.any()) else 1.0
    torch.testing.assert_close(got, want.double(), rtol=tol, atol=tol * max(1.0, peak), equal_nan=True)


def test_refusal_without_a_candidate():
    g, meta = _golden()
    m = meta["empty_replace"]
    assert m["error"] is not None  # (torch reports the zero modulus as a RuntimeError)
    kw = m["kwargs"]
    with pytest.raises(ZeroDivisionError):
        R.restate(torch.from_numpy(g[f"in_{m['input']}"]), kw["quantile"], kw["dim"], True, kw["strategy"], nq_fac=kw["nq_fac"])


def test_mode_takes_the_smallest_of_equally_frequent_values():
    p = torch.tensor([[0.31, 0.29, -1.52, -1.49, 7.0, float("inf"), float("nan")], [float("inf")] * 7])
    mode = R.row_mode(p, 1)
    assert float(mode[0]) == pytest.approx(-1.5) and bool(torch.isnan(mode[1]))
    assert float(R.row_mode(p[:1], 2)) == pytest.approx(-1.52)
