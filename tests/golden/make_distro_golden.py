"""Generates tests/golden/distro_noise.npz by running the REAL reference's DistroNoiseGenerator, its noise item and its
SonarAdvancedDistroNoise node (imported through oracle/ref_import.py) in the build container, in replay mode (cpu=True, seeded with
torch.manual_seed): outputs, and the exception type of every refusal.

    python tests/golden/make_distro_golden.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.ref_import import load_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "distro_noise.npz")
ABI = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "node_abi.json")))["SonarAdvancedDistroNoise"]
ref = load_reference()
FAMILIES = tuple(ref.noise_generation.DistroNoiseGenerator.distro_params().keys())
SHAPE = (2, 4, 10, 14)
VIDEO = (1, 4, 3, 8, 6)

# one non-default parameter set per family (generator keyword arguments, result_index included).  Wishart with d - 1 < df < d makes
# torch resample "singular" draws, a decision taken on the CPU's own rounding: the number of draws consumed would depend on the machine.
VARIANTS = {
    "exponential": dict(exponential_lambd=2.5),
    "cauchy": dict(cauchy_median="0.5", cauchy_sigma=0.3),
    "geometric": dict(geometric_p=0.6),
    "log_normal": dict(log_normal_mean=-0.5, log_normal_std=0.5),
    "normal": dict(normal_mean=1.0, normal_std=3.0),
    "beta": dict(beta_concentration0="0.5 2.0", beta_concentration1="1.5", result_index=(0,)),
    "continuous_bernoulli": dict(continuous_bernoulli_probs="0.2 0.5 0.8", result_index=(0,)),
    "dirichlet": dict(dirichlet_concentration="0.3 0.5 2.0", result_index=(5,)),
    "fisher_snedecor": dict(fisher_snedecor_df1="3.5", fisher_snedecor_df2="5.0"),
    "gamma": dict(gamma_concentration="0.4 3.0", gamma_rate="2.0", result_index=(-2,)),
    "gumbel": dict(gumbel_loc="-1.0", gumbel_scale="0.5"),
    "inverse_gamma": dict(inverse_gamma_concentration="3.0", inverse_gamma_rate="0.5"),
    "kumaraswamy": dict(kumaraswamy_concentration0="2.0", kumaraswamy_concentration1="0.5"),
    "laplacian": dict(laplacian_loc="1.0 -1.0", laplacian_scale="2.0", result_index=(1,)),
    "lkjcholesky": dict(lkjcholesky_dim=4, lkjcholesky_concentration="2.0", result_index=(1, 2)),
    "lrmvariate_normal": dict(lrmvariate_normal_loc="0.0 1.0 2.0", lrmvariate_normal_cov_factor="1.0 0.5 0.0 0.5 -1.0 2.0",
                              lrmvariate_normal_cov_diag="1.0 0.5 2.0", result_index=(1,)),
    "mvariate_normal": dict(mvariate_normal_loc="0.0 2.0 -1.0", mvariate_normal_cov_multiplier=2.0, result_index=(0,)),
    "pareto": dict(pareto_scale="2.0", pareto_alpha="3.0"),
    "poisson": dict(poisson_rate="30.0"),
    "relaxed_bernoulli": dict(relaxed_bernoulli_temperature=0.3, relaxed_bernoulli_probs="0.2"),
    "relaxed_onehotcategorical": dict(relaxed_onehotcategorical_temperature=0.5, relaxed_onehotcategorical_probs="0.1 0.2 0.7",
                                      result_index=(0,)),
    "studentt": dict(studentt_loc="0.5", studentt_scale="2.0", studentt_df="2.7"),
    "uniform": dict(uniform_low=-2.0, uniform_high=3.0),
    "vonmises": dict(vonmises_loc="-2.0", vonmises_concentration="4.0"),
    "weibull": dict(weibull_scale="2.0", weibull_concentration="0.7"),
    "wishart": dict(wishart_cov_size=3, wishart_df="3.5", result_index=(0, -1)),  # df > d: no singular-sample retries
}
assert tuple(VARIANTS) == FAMILIES
MODES = {"global": (None, True), "batch": (0, True), "channel": (1, True), "batch_row": (2, True), "batch_col": (3, True),
         "nonflat_row": (2, False), "nonflat_col": (3, False)}
NODE_FAMILIES = ("uniform", "gamma", "dirichlet", "wishart", "poisson")


def node_defaults(**over):
    kw = {k: v["default"] for k, v in ABI["inputs"].items() if "default" in v}
    kw.update(over)
    return kw


def main():
    arrays, meta = {}, {}
    seed = [100]

    def record(name, entry, fn):
        assert name not in meta, name
        seed[0] += 1
        entry = dict(entry, seed=seed[0], error=None)
        torch.manual_seed(seed[0])
        try:
            outs = fn()
            arrays[name] = torch.stack([o.contiguous() for o in outs]).numpy()
        except Exception as exc:  # noqa: BLE001  (the refusal is the expected result)
            entry["error"] = type(exc).__name__
            entry["message"] = str(exc)[:200]
        meta[name] = entry

    def gen_case(name, shape, calls=1, **kw):
        def run():
            g = ref.noise_generation.DistroNoiseGenerator(torch.zeros(shape), **kw)
            return [g() for _ in range(calls)]

        record(name, {"kind": "generator", "shape": shape, "kwargs": kw, "calls": calls}, run)

    for fam in FAMILIES:
        gen_case(f"default_{fam}", SHAPE, distro=fam, result_index=(-1,))
        gen_case(f"variant_{fam}", SHAPE, distro=fam, **({"result_index": (-1,)} | VARIANTS[fam]))
    for fam in ("gamma", "dirichlet", "normal", "lkjcholesky"):
        gen_case(f"video_{fam}", VIDEO, calls=2, distro=fam, result_index=(-1,))
    for mode, (dim, flat) in MODES.items():
        gen_case(f"mode_{mode}", SHAPE, distro="gumbel", result_index=(-1,), quantile_norm_dim=dim, quantile_norm_flatten=flat)
    gen_case("quantile_negative", SHAPE, distro="laplacian", result_index=(-1,), quantile_norm=-0.7, quantile_norm_pow=0.75,
             quantile_norm_fac=1.3)
    gen_case("quantile_off", SHAPE, distro="exponential", quantile_norm=1.0)
    gen_case("raw_studentt", SHAPE, distro="studentt", result_index=(0,), quantile_norm=1.0, normalized=False)
    # refusals
    gen_case("bad_family", SHAPE, distro="no_such_family")
    gen_case("bad_lambd", SHAPE, distro="exponential", exponential_lambd=-1.0)
    gen_case("multi_simple", SHAPE, distro="normal", normal_mean="0.0 1.0")
    gen_case("wishart_df", SHAPE, distro="wishart", wishart_df="0.5", result_index=(0,))
    gen_case("empty_index", SHAPE, distro="beta", result_index=())

    # the node with its default sockets (and a mode): two calls of its sampler
    def node_case(name, **over):
        def run():
            node = ref.nodes.NODE_CLASS_MAPPINGS["SonarAdvancedDistroNoise"]()
            chain = getattr(node, ABI["function"])(**node_defaults(**over))[0]
            ns = chain.make_noise_sampler(torch.zeros(SHAPE), 0.03, 14.6, seed=7, cpu=True, normalized=True)
            return [ns(torch.tensor(10.0), torch.tensor(5.0)), ns(torch.tensor(5.0), torch.tensor(2.0))]

        record(name, {"kind": "node", "shape": SHAPE, "kwargs": over}, run)

    for fam in NODE_FAMILIES:
        node_case(f"node_{fam}", distribution=fam)
    node_case("node_global", distribution="normal", quantile_norm_mode="global")
    node_case("node_channel", distribution="beta", quantile_norm_mode="channel", result_index="0 1")

    # NoiseType "distro" through CustomNoiseItem with YAML-style parameters
    def item_case(name, params):
        def run():
            item = ref.noise.CustomNoiseItem(0.8, noise_type="distro", ns_kwargs=params)
            ns = item.make_noise_sampler(torch.zeros(SHAPE), 0.03, 14.6, seed=7, cpu=True, normalized=True)
            return [ns(torch.tensor(10.0), torch.tensor(5.0))]

        record(name, {"kind": "item", "shape": SHAPE, "kwargs": params}, run)

    item_case("item_normal", {"distro": "normal", "normal_std": 2.0})
    item_case("item_exponential", {"distro": "exponential", "quantile_norm": 0.9, "quantile_norm_dim": 2})
    item_case("item_gamma_string_index", {"distro": "gamma"})
    item_case("item_gamma_list_index", {"distro": "gamma", "result_index": [0], "gamma_concentration": "2.0"})

    arrays["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    with open(OUT, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    errors = {k: v["error"] for k, v in meta.items() if v["error"]}
    print(f"{os.path.basename(OUT)}  {len(meta)} cases  {os.path.getsize(OUT) / 1024:.1f} KiB  refusals: {errors}")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
