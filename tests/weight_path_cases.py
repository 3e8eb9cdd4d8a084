"""Cases of tests/test_gpu_weight_paths.py: the EM weights of small pairs through the weight kernel (a handle with
SICP_PROFILE_WEIGHT) and through the search's epilogue (a handle without), at the smallest shapes at which either can go wrong:
  n_s  1, 3, 63, 64, 65, 257   ragged quads of the search, a ragged last wave, more than one workgroup of either kernel
  n_t  4, 17, 1000             as few targets as K = 4 allows, fewer than a wave, gathers that spread
  C    1, 2, 11, 16            odd and even projection rows, the longest row the register-resident kernels take
  Probability() as a bool and as a double (quirk_bool_probability 1 / 0: the LITERAL kernels)
  a distance gate at the median d^2 of the pair's slots -- from the points alone, below -- so that about half of them are -1.
run() computes every case of one class count on two handles that live as long as it does."""
from __future__ import annotations

import importlib

import numpy as np

import label_path_cases as cases
import label_path_ref as L

N_S = (1, 3, 63, 64, 65, 257)
N_T = (4, 17, 1000)
CLASSES = (1, 2, 11, 16)
QUIRKS = (1, 0)
PROFILE_WEIGHT = 4  # SICP_PROFILE_WEIGHT: the weight kernel behind the search instead of the search's epilogue


def pair(C, n_t):
    """(src[257], labels, tgt[n_t], labels, qt, gate_sq): the first 257 source points of cases.labelled_pair(C), n_t of its targets
    spread evenly over the cloud; gate_sq = the median float64 d^2 of every source point's 4 nearest targets at qt"""
    src, sl, tgt, tl, qt = cases.labelled_pair(C)
    pick = np.linspace(0, len(tgt) - 1, n_t).astype(int)
    src, sl, tgt, tl = src[:max(N_S)], sl[:max(N_S)], np.ascontiguousarray(tgt[pick]), np.ascontiguousarray(tl[pick])
    q = src.astype(np.float64) @ L.rotation(qt).T + np.asarray(qt)[4:7]
    d2 = ((q[:, None, :] - tgt.astype(np.float64)[None]) ** 2).sum(axis=2)
    gate_sq = float(np.median(np.sort(d2, axis=1)[:, :4]))
    return src, sl, tgt, tl, qt, gate_sq


def key(C, quirk, n_t, n_s, profile):
    return f"C{C}_q{quirk}_t{n_t}_s{n_s}_p{profile}"


def run(C, quirk, reference=False):
    """{key: (idx, w)} of every (n_t, n_s, profile) at this class count and quirk; with `reference`, {key: restatement's w} of
    the profile-0 cases as well, from the engine's own covariances and counts"""
    sicp = importlib.import_module("semantic-icp_amd")
    out, want = {}, {}
    engines = []
    try:
        for profile in (0, PROFILE_WEIGHT):
            p = sicp.default_params(sicp.MODE_EM)
            p.num_classes, p.quirk_bool_probability, p.profile = C, quirk, profile
            e = sicp.Engine(0, p)
            engines.append(e)
            e.set_confusion(cases.matrix(C))
        for n_t in N_T:
            src, sl, tgt, tl, qt, gate_sq = pair(C, n_t)
            for e in engines:
                p = e.get_params()
                p.gate_sq = gate_sq
                e.set_params(p)
                e.set_target(tgt, tl)
            for n_s in N_S:
                for e, profile in zip(engines, (0, PROFILE_WEIGHT)):
                    e.set_source(src[:n_s], sl[:n_s])
                    st0 = e.stats()
                    idx, _, w = e.correspondences(qt)
                    st1 = e.stats()
                    # the counters say which kernel wrote the weights
                    assert st1["weights_in_search"] - st0["weights_in_search"] == (0 if profile else 1)
                    assert st1["weight_launches"] - st0["weight_launches"] == (1 if profile else 0)
                    out[key(C, quirk, n_t, n_s, profile)] = (idx, w)
                    if reference and profile == 0:
                        scov, _, sh, _ = e.covariances(sicp.SOURCE, want_hist=True)
                        tcov, _, th, _ = e.covariances(sicp.TARGET, want_hist=True)
                        want[key(C, quirk, n_t, n_s, 0)] = L.weights(sh, th, cases.matrix(C), cases.K_COV, qt, src[:n_s], scov, tgt, tcov, idx,
                                                                    as_bool=bool(quirk))
    finally:
        for e in engines:
            e.close()
    return (out, want) if reference else out

