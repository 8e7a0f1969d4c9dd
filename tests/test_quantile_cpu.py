"""CPU: the quantile filter's host side -- the strategy table against the node ABI, node registration, argument refusals raised before any
kernel launch, and the fp32 rank split against torch.quantile."""
import importlib
import json
import os

import pytest
import torch

from tests.conftest import GOLDEN

ABI = json.load(open(os.path.join(GOLDEN, "node_abi.json")))


def _utils(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.utils")


def test_strategy_table_is_the_dropdown(pkg):
    utils = _utils(pkg)
    for key in ("SonarQuantileFilteredNoise", "SonarLatentOperationQuantileFilter"):
        assert tuple(utils.quantile_handlers.keys()) == tuple(ABI[key]["inputs"]["strategy"]["type"])
    assert len(utils.quantile_handlers) == 43


def test_both_nodes_are_implemented(pkg):
    reg = importlib.import_module("comfyui_sonar_amd.py.nodes.registry")
    for key in ("SonarQuantileFilteredNoise", "SonarLatentOperationQuantileFilter"):
        assert key in reg.IMPLEMENTED_KEYS
        assert not reg.NODE_CLASS_MAPPINGS[key].__name__.startswith("OffPath_")


def test_refusals_come_before_any_launch(pkg):
    """CPU tensors: each refusal is the reference's exception type, raised before the device check (which would raise SonarHipError)."""
    utils = _utils(pkg)
    x = torch.randn(2, 4, 6, 5)
    with pytest.raises(TypeError):
        utils.quantile_normalize(x, dim=None, flatten=True)
    with pytest.raises(ValueError):
        utils.quantile_normalize(x, strategy="no_such_strategy")
    with pytest.raises(IndexError):
        utils.quantile_normalize(x, dim=4, flatten=True)
    with pytest.raises(IndexError):
        utils.quantile_normalize(x, dim=4, flatten=False)
    for s in ("median", "mode_1dec", "mode_2dec", "scale_down"):
        with pytest.raises(RuntimeError):
            utils.quantile_normalize(x, dim=None, flatten=False, strategy=s)
    with pytest.raises(NotImplementedError):
        utils.quantile_normalize(x, strategy_handler=lambda noise, nq, **kw: noise)
    # early returns hand back the very same tensor
    for q in (None, 1.0, -1.0, 1.5):
        assert utils.quantile_normalize(x, quantile=q) is x
    e = torch.empty(0, 4)
    assert utils.quantile_normalize(e) is e
    # a launchable call on a CPU tensor fails loudly instead of falling back
    hl = pkg.hip_lib
    with pytest.raises(hl.SonarHipError):
        utils.quantile_normalize(x)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 100, 140, 560, 4097, 65536, 262144, 1 << 20])
def test_rank_split_matches_torch(pkg, n):
    hl = pkg.hip_lib
    ramp = torch.arange(n, dtype=torch.float32) if n <= (1 << 16) else None
    for q in (0.0, 0.1, 0.25, 0.5, 0.7, 0.75, 0.85, 0.9, 0.99, 0.999999):
        lo, frac = hl.quantile_rank(q, n)
        assert 0 <= lo < n and 0.0 <= frac <= 1.0
        rank = torch.tensor(q, dtype=torch.float32) * (n - 1)
        assert lo == min(int(torch.floor(rank)), n - 1)
        if ramp is not None:  # the order statistics of a ramp are their ranks: torch.quantile returns lo + frac
            want = float(torch.quantile(ramp, q))
            got = float(torch.lerp(torch.tensor(float(lo)), torch.tensor(float(min(lo + 1, n - 1))), torch.tensor(frac)))
            assert got == pytest.approx(want, rel=1e-6, abs=1e-6)


def test_strategy_codes_match_the_header(pkg):
    import re

    hl = pkg.hip_lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "sonar_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define SONAR_(Q_\w+) (0x[0-9a-fA-F]+|\d+)", header)}
    assert len(defs) == 21
    for name, val in defs.items():
        assert getattr(hl, name) == val, name
