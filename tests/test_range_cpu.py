"""CPU tests of the range image's rules: tests/range_ref.py, the numpy restatement the GPU tests compare to the bit, against
independent formulations -- arctan2 / arcsin / floor in float64 for the projection, the RangeNet++ column formula, a brute-force
k-d tree restricted to the window for the vote -- and the host-only entry points sicp_default_range_params / sicp_range_tables
against the same formulas in numpy."""
import importlib

import numpy as np
import pytest

import range_cases
import range_ref as R

sicp = importlib.import_module("semantic-icp_amd")
INV = sicp.ERR_INVALID_ARGUMENT
MARGIN = 1e-6  # rad: a point nearer than this to an edge may fall to either side of it in float64 too


def _cloud(seed):
    """20 000 seeded points well inside the range bounds (so that only the angles decide)"""
    xyz, _ = range_cases.sphere(20000, seed, r_lo=1.0, r_hi=100.0, el_lo=-0.5, el_hi=0.1)
    return xyz


def _independent(xyz, p):
    """azimuth, elevation, sector, row and the distance to the nearest edge of either kind, all in float64"""
    q = xyz.astype(np.float64)
    W, H = p.width, p.height
    az = np.arctan2(q[:, 1], q[:, 0]) % (2.0 * np.pi)
    el = np.arcsin(q[:, 2] / np.sqrt((q * q).sum(axis=1)))
    u = az * W / (2.0 * np.pi)
    sector = np.floor(u).astype(np.int64) % W
    d_az = np.abs(u - np.round(u)) * (2.0 * np.pi / W)
    v = (p.fov_up - el) * H / (p.fov_up - p.fov_down)
    row = np.floor(v).astype(np.int64)
    d_el = np.abs(v - np.round(v)) * ((p.fov_up - p.fov_down) / H)
    return az, el, sector, row, np.minimum(d_az, d_el)


@pytest.mark.parametrize("W,H", [(64, 5), (2048, 64)])
def test_the_restatement_equals_arctan2_arcsin_floor(W, H):
    p = R.params(width=W, height=H, min_range=0.5, max_range=120.0)
    xyz = _cloud(7 + W)
    pr = R.project(xyz, p, R.tables(p))
    az, el, sector, row, dist = _independent(xyz, p)
    safe = dist > MARGIN
    left_out = 1.0 - safe.mean()
    expected = W * 2 * MARGIN / (2 * np.pi) + H * 2 * MARGIN / (p.fov_up - p.fov_down)
    print("left out by the margin:", left_out, "expected about", expected)
    assert left_out <= 0.01
    assert pr["kept"].all()
    inside = (row >= 0) & (row < H)
    assert inside[safe].sum() > 10000
    assert (pr["inview"][safe] == inside[safe]).all()
    assert (pr["sector"][safe] == sector[safe]).all()
    both = safe & inside
    assert (pr["row"][both] == row[both]).all()
    col = ((W - 1 - sector) + p.col_shift) % W
    assert (pr["pixel"][both] == row[both] * W + col[both]).all()


@pytest.mark.parametrize("W,H", [(64, 5), (2048, 64)])
def test_clockwise_with_half_a_turn_is_the_rangenet_column(W, H):
    p = R.params(width=W, height=H, clockwise=1, col_shift=W // 2, min_range=0.5, max_range=120.0)
    xyz = _cloud(7 + W)
    pr = R.project(xyz, p, R.tables(p))
    q = xyz.astype(np.float64)
    yaw = -np.arctan2(q[:, 1], q[:, 0])
    u = 0.5 * (yaw / np.pi + 1.0) * W  # proj_x of the RangeNet++ / SemanticKITTI laserscan: 0.5 (yaw / pi + 1) W, yaw = -atan2(y, x)
    want = np.clip(np.floor(u), 0, W - 1).astype(np.int64)
    safe = np.abs(u - np.round(u)) * (2.0 * np.pi / W) > MARGIN
    assert safe.mean() >= 0.99
    assert (pr["col"][safe] == want[safe]).all()
    # and the issue's form of it
    assert (np.floor(0.5 * (1.0 - np.arctan2(q[:, 1], q[:, 0]) / np.pi) * W)[safe] % W == pr["col"][safe]).all()


def test_the_vote_equals_a_kd_tree_restricted_to_the_window():
    from scipy.spatial import cKDTree

    c = range_cases.vote_case(seed=41, n=1200, W=24, H=5)
    for S, K in ((3, 3), (5, 5), (7, 16), (1, 4)):
        p = R.params(**dict(c["p"], window=S, k=K))
        tab = R.tables(p)
        got = R.vote(c["xyz"], c["labels"], c["pixel_label"], p, tab)
        im = got["image"]
        W, H = p.width, p.height
        win = im["index"].reshape(-1)
        xyz64 = c["xyz"].astype(np.float64)
        checked = 0
        for i in np.flatnonzero(im["pixel"] >= 0):
            r, col = divmod(int(im["pixel"][i]), W)
            cand = [rr * W + (col + wc) % W for rr in range(r - S // 2, r + S // 2 + 1) if 0 <= rr < H
                    for wc in range(-(S // 2), S // 2 + 1)]
            cand = [q for q in cand if win[q] >= 0]
            tree = cKDTree(xyz64[win[cand]])
            d, j = tree.query(xyz64[i], k=min(K, len(cand)), distance_upper_bound=np.sqrt(p.max_dist_sq))
            d, j = np.atleast_1d(d), np.atleast_1d(j)
            j = j[np.isfinite(d)]
            d = d[np.isfinite(d)]
            if len(d) > 1 and np.min(np.diff(np.sort(d))) < 1e-4:
                continue  # (a near tie in distance: float32 and float64 may order it differently)
            if len(d) and abs(d.max() ** 2 - p.max_dist_sq) < 1e-3:
                continue
            classes = c["pixel_label"].reshape(-1)[np.array(cand, dtype=np.int64)[j]] if len(j) else np.zeros(0, np.uint32)
            classes = classes[classes != 0]
            assert got["neighbours"][i] == len(d), (S, K, i)
            if len(classes) == 0:
                assert got["votes"][i] == 0 and got["labels"][i] == c["labels"][i]
            else:
                vals, cnt = np.unique(classes, return_counts=True)
                assert got["labels"][i] == vals[np.argmax(cnt)] and got["votes"][i] == cnt.max()  # (argmax: the smallest label of a tie)
            checked += 1
        print("window", S, "k", K, "points checked", checked, "of", int((im["pixel"] >= 0).sum()))
        assert checked > 0.9 * (im["pixel"] >= 0).sum()


def test_beam_table_edges():
    """an uneven table: inner edges at the midpoints, outer edges half the neighbouring gap beyond; H = 1: the field of view"""
    beam = np.array([0.20, 0.10, 0.05, -0.10, -0.40])
    p = sicp.default_range_params(width=16, height=5)
    tab = sicp.range_tables(p, beam)
    a = np.array([0.25, 0.15, 0.075, -0.025, -0.25, -0.55])
    assert np.allclose(R.edge_angles(p, beam), a, rtol=0, atol=1e-15)
    want = np.tan(a) * np.abs(np.tan(a))
    assert np.allclose(tab["row_edge"], want, rtol=1e-14, atol=0)
    assert (np.diff(tab["row_edge"]) < 0).all()
    assert np.allclose(tab["row_edge"], R.tables(p, beam)["row_edge"], rtol=1e-14, atol=0)
    one = sicp.default_range_params(width=16, height=1, fov_up=0.3, fov_down=-0.2)
    t1 = sicp.range_tables(one, np.array([0.0]))["row_edge"]
    assert np.allclose(t1, [np.tan(0.3) ** 2, -np.tan(0.2) ** 2], rtol=1e-14, atol=0)
    assert t1.tobytes() == sicp.range_tables(one)["row_edge"].tobytes()


def test_default_params_and_tables():
    p = sicp.default_range_params()
    assert (p.width, p.height, p.clockwise, p.col_shift, p.window, p.k) == (2048, 64, 1, 1024, 5, 5)
    assert (p.min_range, p.max_range, p.max_dist_sq) == (0.5, 120.0, 1.0)
    assert abs(p.fov_up - np.deg2rad(3.0)) < 1e-15 and abs(p.fov_down + np.deg2rad(25.0)) < 1e-15
    q = R.params()
    assert all(getattr(p, k) == pytest.approx(getattr(q, k), abs=1e-15) for k in vars(q))
    assert sicp.default_range_params(width=24).col_shift == 12
    for W, H in ((16, 1), (24, 5), (4096, 256)):
        pp = sicp.default_range_params(width=W, height=H)
        tab, ref = sicp.range_tables(pp), R.tables(pp)
        assert tab["cos_half"].shape == (W // 2,) and tab["row_edge"].shape == (H + 1,)
        assert tab["row_edge"][0] > 0 > tab["row_edge"][H]
        for k in ref:
            assert np.abs(tab[k] - ref[k]).max() <= 4 * np.finfo(np.float64).eps, k  # (libm against numpy: an ulp or two at most)
    # an inner edge at elevation 0 exactly
    assert sicp.range_tables(sicp.default_range_params(width=16, height=2, fov_up=0.3, fov_down=-0.3))["row_edge"][1] == 0.0


@pytest.mark.parametrize("kw,beam", [
    (dict(width=17), None), (dict(width=14), None), (dict(width=4098), None), (dict(height=0), None), (dict(height=257), None),
    (dict(fov_up=-0.5), None), (dict(fov_up=0.1, fov_down=0.1), None), (dict(fov_up=np.pi / 2), None), (dict(fov_down=-np.pi / 2), None),
    (dict(fov_up=np.nan), None), (dict(min_range=-1.0), None), (dict(max_range=0.5), None), (dict(max_range=np.inf), None),
    (dict(clockwise=2), None), (dict(col_shift=-1), None), (dict(width=16, col_shift=16), None), (dict(window=4), None),
    (dict(window=9), None), (dict(window=0), None), (dict(k=0), None), (dict(k=17), None), (dict(max_dist_sq=-1.0), None),
    (dict(max_dist_sq=np.nan), None),
    (dict(height=3), [-0.1, 0.0, 0.1]), (dict(height=3), [0.1, 0.1, 0.0]), (dict(height=3), [0.1, np.nan, -0.1]),
    (dict(height=2), [1.5, 0.0]),
])
def test_tables_refuse_bad_parameters(kw, beam):
    p = sicp.default_range_params(**kw)
    with pytest.raises(sicp.SicpError) as err:
        sicp.range_tables(p, None if beam is None else np.array(beam))
    assert err.value.status == INV
