#!/usr/bin/env python3
"""Golden fixtures for the ASV evaluation (satools_amd.asv_eval, csrc/asv_score.hip): runs the REFERENCE's own
`scoring.cosine_scoring`, `scoring.asnorm`, `scoring.linkability` and `scoring.min_cllr(..., compute_eer=True, return_opt=True)`
(satools/sidekit/scoring) on seeded synthetic data and stores inputs and outputs in fx_asv_eval.npz.  Only recorded data is kept.

The scoring package imports the third-party `feerci` at the top; it is not installed, none of the four functions uses it, and a
placeholder module stands in for the import (parity unpinned).

Vector cases (`c50_t300`, `c1000_t5000`): D = 192; a speaker is a random centre, an utterance the centre plus noise, normalised, so
that mated scores exceed non-mated ones but overlap.  S enrolment speakers (their vectors: normalised means of three utterances),
T test utterances, every (speaker, utterance) pair a trial.  The cohort is stored as float16 (its values are exact in float32;
asnorm takes plain dot products, so nearly-unit rows serve) to keep the file under the size limit.
Score-only cases: `separated` (no overlap), `tied` (scores on a grid of 0.05: many exact ties within and across the sets),
`few_mated` (15 mated scores: one linkability bin).
`c50_t300` is searched over seeds until no target / non-target pair of scores and no score / histogram-edge pair is closer than
MARGIN (raw) or MARGIN_AS (after s-norm): tests/test_hip_asv_score.py compares the metrics of the device's scores with the
recorded ones, which only holds to rounding when the order of the scores and their bins cannot change.
     python tests/golden/make_asv_eval_fixtures.py"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as mf   # noqa: E402

MARGIN, MARGIN_AS = 2e-5, 1.5e-3


def load_scoring(ref):
    stub = types.ModuleType("feerci")
    stub.feerci = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("feerci is not installed"))
    sys.modules.setdefault("feerci", stub)
    if not hasattr(np, "trapz"):
        np.trapz = np.trapezoid
    d = os.path.join(ref, "satools", "satools", "sidekit", "scoring")
    spec = importlib.util.spec_from_file_location("ref_scoring", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_scoring"] = mod
    spec.loader.exec_module(mod)
    return mod


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def vectors(seed, S, T, C, D=192, noise=5.0):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(S, D, generator=g)
    utt = lambda c: unit(c + noise * torch.randn(c.shape, generator=g))
    enroll = unit(torch.stack([utt(centres) for _ in range(3)]).mean(0))
    owner = torch.arange(T) % S
    test = utt(centres[owner])
    cohort = unit(torch.randn(C, D, generator=g) + 0.5 * centres[torch.arange(C) % S]).to(torch.float16)
    return enroll.float(), test.float(), cohort, owner.numpy()


def metrics_of(sc, mated, non):
    out = {"linkability": np.float64(sc.linkability(mated, non)[0])}
    cmin, eer, tar, nontar = sc.min_cllr(mated, non, compute_eer=True, return_opt=True)
    out.update(min_cllr=np.float64(cmin), eer=np.float64(eer), tar_llrs=np.asarray(tar), non_llrs=np.asarray(nontar))
    return out


def min_gaps(mated, non):
    """(smallest |target - non-target| score difference, smallest distance of a score to an inner histogram edge)"""
    gap = np.abs(mated[:, None] - non[None, :]).min()
    n_bins = min(int(len(mated) / 10), 100)
    both = np.concatenate([mated, non])
    edges = np.linspace(both.min(), both.max(), n_bins + 1)[1:-1]
    return gap, (np.abs(both[:, None] - edges[None, :]).min() if len(edges) else np.inf)


def vector_case(sc, seed, S, T, C):
    enroll, test, cohort, owner = vectors(seed, S, T, C)
    idx_e = np.repeat(np.arange(S), T).astype(np.int32)
    idx_t = np.tile(np.arange(T), S).astype(np.int32)
    target = owner[idx_t] == idx_e
    e_xv, t_xv = enroll[idx_e], test[idx_t]
    scores = np.asarray(sc.cosine_scoring(list(e_xv.numpy()), list(t_xv.numpy())), dtype=np.float64)
    as_scores = sc.asnorm(torch.FloatTensor(list(scores)), e_xv, t_xv, cohort.float()).numpy()
    out = {"enroll": enroll.numpy(), "test": test.numpy(), "cohort_f16": cohort.numpy(), "idx_e": idx_e, "idx_t": idx_t, "target": target,
           "scores": scores, "asnorm": as_scores}
    for tag, s in (("raw", scores), ("as", as_scores.astype(np.float64))):
        for k, v in metrics_of(sc, s[target], s[~target]).items():
            out[f"{tag}/{k}"] = v
    return out


def score_case(sc, mated, non):
    out = {"mated": mated, "non": non}
    out.update(metrics_of(sc, mated, non))
    return out


def main():
    ref = mf.setup_reference()
    sc = load_scoring(ref)
    cases = {}
    for seed in range(1000, 5000):
        c = vector_case(sc, seed, 15, 20, 50)
        t = c["target"]
        ok = all(min(min_gaps(s[t], s[~t])) > m for s, m in ((c["scores"], MARGIN), (c["asnorm"].astype(np.float64), MARGIN_AS)))
        if ok:
            print("c50_t300: seed", seed)
            c["seed"] = np.int64(seed)
            cases["c50_t300"] = c
            break
    else:
        raise SystemExit("no seed gives the margins")
    cases["c1000_t5000"] = vector_case(sc, 7, 20, 250, 1000)
    rng = np.random.default_rng(3)
    cases["separated"] = score_case(sc, 0.6 + 0.1 * rng.random(120), -0.1 + 0.3 * rng.random(900))
    cases["tied"] = score_case(sc, np.round((0.35 + 0.2 * rng.standard_normal(200)) / 0.05) * 0.05,
                               np.round((0.05 + 0.2 * rng.standard_normal(1500)) / 0.05) * 0.05)
    cases["few_mated"] = score_case(sc, 0.3 + 0.2 * rng.standard_normal(15), 0.2 * rng.standard_normal(200))
    flat = {f"{name}/{k}": v for name, c in cases.items() for k, v in c.items()}
    path = os.path.join(HERE, "fx_asv_eval.npz")
    np.savez_compressed(path, **flat)
    for name, c in cases.items():
        print(name, {k: (v.shape if getattr(v, "ndim", 0) else float(v)) for k, v in c.items()})
    print(os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
