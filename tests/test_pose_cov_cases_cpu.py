"""CPU tests of what tests/test_gpu_pose_cov_paths.py stands on (tests/pose_cov_cases.py, tests/pose_cov_ref.py): every
crafted pair gives the oracle's k-NN exactly the run lengths and the gated count its case claims; the interval model of
the tile and owner rule agrees with a literal walk of the two kernels' loops; the restatement's derivatives match central
differences of lm_ref's gradient for both loss stacks with weights present and absent; its float64 and longdouble runs
agree; and -- on the reference alone -- no geometry case could lose a piece of a run under the bar."""
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import lm_ref
import oracle_lib as O
import pose_cov_cases as P
import pose_cov_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3


def test_tile_size_is_the_header_s():
    src = open(os.path.join(ROOT, "semantic-icp_amd", "csrc", "kernels.h")).read()
    m = re.search(r"constexpr\s+int\s+kPoseCovTile\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == P.TILE
    assert re.search(r"pose_cov_blocks\(int items\)[^}]*\(items \+ 255\) / 256", src)  # LANES: 256 tiles per workgroup
    assert P.LANES == 256
    assert np.finfo(np.longdouble).eps < 1e-18  # the restatement's second run is wider than float64


# ---- the tile and owner rule, walked literally ------------------------------------------------------------------------------------
FIRST_CONTINUES, OWNS_LAST, PASS_THROUGH = 1, 2, 4


def walk(run_lengths, gated, tile, lanes):
    """pose_cov_tile_jobs' loop over every tile of an explicit array of sorted targets (-1 = gated out), then
    pose_cov_owner_jobs' walk over the flags; counts under tile_geometry's names"""
    tg = np.concatenate([np.full(n, r) for r, n in enumerate(run_lengths)] + [np.full(gated, -1)]).astype(np.int64)
    total = len(tg)
    tiles = (total + tile - 1) // tile
    flags = np.zeros(tiles, dtype=int)
    inside = 0
    for t in range(tiles):
        b, e = t * tile, min((t + 1) * tile, total)
        prev = tg[b - 1] if b > 0 else -2
        nxt = tg[e] if e < total else -2
        cur, start, pos = -1, b, b

        def finish(end):
            nonlocal inside
            cin, cout = start == b and cur == prev, end == e and cur == nxt
            if not cin and not cout:
                inside += 1
            else:
                flags[t] |= (FIRST_CONTINUES | (PASS_THROUGH if cout else 0)) if cin else OWNS_LAST

        while pos < e:
            if tg[pos] < 0:
                break
            if tg[pos] != cur:
                if cur >= 0:
                    finish(pos)
                cur, start = tg[pos], pos
            pos += 1
        if cur >= 0:
            finish(pos)
    chains = []
    for t in range(tiles):
        if flags[t] & OWNS_LAST:
            u = t + 1
            while u < tiles:
                assert flags[u] & FIRST_CONTINUES
                if not flags[u] & PASS_THROUGH:
                    break
                u += 1
            assert u < tiles
            chains.append((t, u))
    live = int(sum(run_lengths))
    ends = np.cumsum(run_lengths)
    starts = ends - np.asarray(run_lengths)
    return dict(inside=inside, owns_last=int((flags & OWNS_LAST > 0).sum()), first_continues=int((flags & FIRST_CONTINUES > 0).sum()),
                pass_through=int((flags & PASS_THROUGH > 0).sum()), crossing_workgroup=sum(t // lanes != u // lanes for t, u in chains),
                through_workgroup=sum(u // lanes - t // lanes >= 2 for t, u in chains), longest_chain=max([u - t + 1 for t, u in chains] or [1 if live else 0]),
                ends_on_edge=int((ends % tile == 0).sum()), start_phases=len(set((starts % tile).tolist())),
                gated_on_edge=int(gated > 0 and live % tile == 0), gated_beside_edge=int(gated > 0 and live % tile in (1, tile - 1)),
                tiles=tiles, workgroups=(tiles + lanes - 1) // lanes)


@pytest.mark.parametrize("seed", range(6))
def test_tile_geometry_equals_a_literal_walk(seed):
    rng = np.random.default_rng(seed)
    for trial in range(40):
        tile, lanes = (P.TILE, P.LANES) if trial % 2 == 0 else (int(rng.integers(1, 6)), int(rng.integers(1, 5)))
        longest = int(rng.choice([3, 12, 40, 3 * tile * lanes]))
        runs = rng.integers(1, longest + 1, int(rng.integers(0, 30))).tolist()
        gated = int(rng.choice([0, 0, 1, tile - 1, tile, tile + 1, 50]))
        if not runs and gated == 0:
            continue
        assert P.tile_geometry(runs, gated, tile, lanes) == walk(runs, gated, tile, lanes), (runs, gated, tile, lanes)


def test_every_case_reaches_the_path_it_claims():
    seen = {}
    for case in P.GEOMETRY_CASES:
        n_s, n_t, live, gated = P.slots_of_case(case)
        geo = P.tile_geometry([case.L] * (case.T * case.K), gated)
        P.check_claims(case, geo)
        assert n_s * case.K <= 10200 and n_s <= 10200, case.name
        for k, v in geo.items():
            seen[k] = max(seen.get(k, 0), v)
    assert seen["crossing_workgroup"] >= 3 and seen["through_workgroup"] >= 1 and seen["longest_chain"] >= 513
    assert seen["gated_on_edge"] == 1 and seen["gated_beside_edge"] == 1 and seen["pass_through"] >= 256
    names = set(P.GEOMETRY)
    assert {f"T37_K1_L{L}_g0" for L in (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65)} <= names
    assert {f"T3_K1_L{L}_g0" for L in (2047, 2048, 2049)} | {"T2_K1_L4104_g0"} <= names
    assert {f"T37_K{K}_L{L}_g0" for K in (4, 20) for L in (7, 8, 9)} <= names
    assert {f"T37_K1_L{L}_g{g}" for L in (8, 9) for g in (0, 1, 7, 8, 9)} <= names
    powers = [P.slots_of_case(c) for c in P.GEOMETRY_CASES]
    assert any(n_t == 64 for _, n_t, _, _ in powers) and any(live + gated == 2048 for _, _, live, gated in powers)
    assert any(n_t == 64 and gated for _, n_t, _, gated in powers) and any(live + gated == 2048 and gated for _, _, live, gated in powers)


# ---- the crafted pairs under the oracle's search ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.GEOMETRY))
def test_oracle_knn_gives_the_claimed_runs(name):
    case = P.GEOMETRY[name]
    src, sl, tgt, tl = P.case_pair(case)
    n_s, n_t, live, gated = P.slots_of_case(case)
    assert src.shape == (n_s, 3) and tgt.shape == (n_t, 3) and np.abs(src).max() < 1000 and np.abs(tgt).max() < 1000
    idx, d2 = O.knn(src, tgt, case.K, kdtree=True)
    idx = np.where(d2 <= P.GATE_SQ, idx, -1)
    runs, dead = P.run_lengths_of(idx, n_t)
    assert dead == gated and len(runs) == n_t and (runs == case.L).all()
    assert ((idx < 0).all(axis=1) | (idx >= 0).all(axis=1)).all()          # a source point is gated as a whole
    assert d2[idx >= 0].max() < 1.0 and (gated == 0 or d2[idx < 0].min() > 1600.0)
    if case.K > 1:   # a point's K slots hit K different targets: its slots lie in K different runs
        assert all(len(set(row)) == case.K for row in idx[(idx >= 0).all(axis=1)][:50].tolist())


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _random_slots(rng, n):
    def unit(m):
        v = rng.normal(size=(m, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    p = rng.uniform(-5, 5, size=(n, 3))
    return p, unit(n), p + rng.normal(scale=0.3, size=(n, 3)), unit(n)


def _pose(rng):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(rng.normal(scale=0.4, size=3)).as_matrix()
    T[:3, 3] = rng.normal(scale=0.5, size=3)
    return T


@pytest.mark.parametrize("a", [0.5, 3.0])
@pytest.mark.parametrize("weighted", [0, 1])
@pytest.mark.parametrize("sq", [0, 1])
def test_both_stacks_match_central_differences(sq, weighted, a):
    """B^p and B^q of 48 slots against central differences of lm_ref's per-slot gradient; lm_ref.loss states the weight rule
    on its own (no ScaledLoss around the bare Cauchy), the restatement through effective_weights"""
    rng = np.random.default_rng(100 + 4 * sq + 2 * weighted + int(a))
    n = 48
    T = _pose(rng)
    p, ns, q, nt = _random_slots(rng, n)
    w = rng.uniform(0.2, 1.0, size=n) if weighted else None
    ww = ref.effective_weights(w, sq, n)
    assert (ww == 1).all() if not (sq and weighted) else np.array_equal(ww, w)
    _, _, Bp, Bq = ref.slot_terms(T[:3, :3], T[:3, 3], p, ns, q, nt, EPS, None, a, ww, use_sqloss=sq)
    pairs = np.stack([np.arange(n), np.arange(n)], 1)

    def grads(pp, qq):
        r, J = lm_ref.residuals_and_jacobian(T, pp, ns, qq, nt, pairs, EPS)
        _, drho = lm_ref.loss(None, r * r, np.ones(n) if w is None else w, a, use_sqloss=sq)
        return (drho * r)[:, None] * J

    h = 1e-6
    for z, B in (("p", Bp), ("q", Bq)):
        fd = np.zeros_like(B)
        for col in range(3):
            e = np.zeros(3)
            e[col] = h
            fd[:, :, col] = ((grads(p + e, q) - grads(p - e, q)) if z == "p" else (grads(p, q + e) - grads(p, q - e))) / (2 * h)
        scale = np.abs(fd).max(axis=(1, 2), keepdims=True) + 1e-12
        assert (np.abs(B - fd) / scale).max() < 1e-5, (sq, weighted, a, z)
    if weighted:  # the weights do change the SQLoss stack's terms, and would change the Cauchy's if they were applied
        _, _, _, other = ref.slot_terms(T[:3, :3], T[:3, 3], p, ns, q, nt, EPS, None, a, ref.effective_weights(w, sq, n, always=True) if not sq
                                        else np.ones(n), use_sqloss=sq)
        assert np.abs(other - Bq).max() > 1e-2 * np.abs(Bq).max()


def test_mode_names_keep_their_default_stacks():
    rng = np.random.default_rng(5)
    s, w = rng.uniform(0, 4, 20), rng.uniform(0.2, 1, 20)
    for mode, (sq, a) in ref.STACKS.items():
        for x, y in zip(ref.rho1_kappa(mode, s, w, a), ref.rho1_kappa(None, s, w, a, use_sqloss=sq)):
            assert np.array_equal(x, y)
        lo = lm_ref.loss(mode, s, w, a)
        ln = lm_ref.loss(None, s, w if mode == "em" else np.ones(20), a, use_sqloss=sq)
        assert np.array_equal(lo[0], ln[0]) and np.array_equal(lo[1], ln[1])


@pytest.mark.parametrize("sq,a,eps", [(1, 3.0, 1e-3), (0, 1.5, 1e-3), (1, 0.5, 1e-2), (0, 10.0, 1e-6), (1, 3.0, 1e-6)])
def test_longdouble_run_agrees_with_float64(sq, a, eps):
    """random slots with shared targets and weights: the two runs of cross_sums agree to float64's own error in these
    formulas (the closed-form 3x3 inverse against np.linalg.inv included)"""
    rng = np.random.default_rng(11)
    n_s, n_t, K = 60, 25, 4
    src, sn, _, _ = _random_slots(rng, n_s)
    tgt, tn, _, _ = _random_slots(rng, n_t)
    idx = rng.integers(0, n_t, (n_s, K)).astype(np.int32)
    idx[::9, 1] = -1
    w = rng.uniform(0.1, 1.0, (n_s, K))
    T = _pose(rng)
    qt = np.concatenate([Rotation.from_matrix(T[:3, :3]).as_quat(), T[:3, 3]])
    want, gaps = P.reference(qt, src, sn, tgt, tn, idx, w, eps, sq, a)
    print(f"sqloss {sq} a {a} eps {eps}: float64 to longdouble {gaps[0]:.2e} (source) {gaps[1]:.2e} (target)")
    assert max(gaps) < (1e-9 if eps >= 1e-3 else 1e-5)
    assert np.abs(P.rotation(qt) - T[:3, :3]).max() < 1e-15
    direct = ref.cross_sums(P.rotation(qt), T[:3, 3], src, sn, tgt, tn, idx, w, eps, None, a, use_sqloss=sq)
    assert np.array_equal(direct[0], want[0]) and np.array_equal(direct[1], want[1])
    A = rng.normal(size=(7, 3, 3)) + 3 * np.eye(3)
    assert np.abs(ref.inv3(A) @ A - np.eye(3)).max() < 1e-12
    assert np.abs(ref.inv3(A.astype(np.longdouble)) @ A - np.eye(3)).max() < 1e-16


# ---- would the bar hide a lost piece? -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.GEOMETRY))
def test_a_lost_piece_moves_the_reference_beyond_the_bar(name):
    """normals from the oracle's covariances, the oracle's neighbours under the identity pose, the default EM stack: S_tgt
    without the part of ONE run that lies beyond its first tile edge (whichever target that run belongs to, whichever of the
    case's pieces it is; a whole run where no run crosses an edge) differs by more than 100 bars"""
    case = P.GEOMETRY[name]
    src, sl, tgt, tl = P.case_pair(case)
    sn = O.covariances(src, None, 20, EPS, kdtree=True)[1]
    tn = O.covariances(tgt, None, 20, EPS, kdtree=True)[1]
    idx, d2 = O.knn(src, tgt, case.K, kdtree=True)
    idx = np.where(d2 <= P.GATE_SQ, idx, -1).astype(np.int32)
    _, gaps = P.reference(P.IDENT, src, sn, tgt, tn, idx, None, EPS, 1, 3.0)
    bar = P.bar_of(gaps[1])
    least = P.least_movement(P.IDENT, src, sn, tgt, tn, idx, EPS, 1, 3.0, P.lost_pieces(case))
    print(f"{name}: pieces {P.lost_pieces(case)}, least movement {least:.3e}, bar {bar:.3e}")
    assert np.isfinite(least) and least > 100 * bar, (name, least, bar)
