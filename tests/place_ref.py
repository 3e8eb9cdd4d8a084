"""The numpy restatement of sicp_place_* (include/sicp.h, rules 1-6): the specification's twin.  Every function takes the three
tables as arguments; make_tables() builds them with math.cos / math.sin (libm), as the library's host code does.  Ranking is
with fractions.Fraction; key30() is the integer sort key the device uses."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

LABEL, HEIGHT = 0, 1
TWO_PI = 6.283185307179586


class BadLabel(Exception):
    """a kept point's label above num_classes (SICP_ERR_BAD_LABEL)"""


def make_tables(R: int, S: int, max_range: float):
    """rule 2: {"edge2": [R+1], "cos_half": [S/2], "sin_half": [S/2]} in float64, element by element with libm"""
    ring_step = max_range / float(R)
    sector_step = TWO_PI / float(S)
    edge2 = np.array([(float(i) * ring_step) * (float(i) * ring_step) for i in range(R + 1)], dtype=np.float64)
    cos_half = np.array([math.cos(float(j) * sector_step) for j in range(S // 2)], dtype=np.float64)
    sin_half = np.array([math.sin(float(j) * sector_step) for j in range(S // 2)], dtype=np.float64)
    return {"edge2": edge2, "cos_half": cos_half, "sin_half": sin_half}


def params(R=20, S=60, max_range=40.0, min_range=0.0, channel=LABEL, num_classes=0, z_min=-2.0, z_step=0.5, min_cell_points=1,
           ignore=()):
    return dict(R=R, S=S, max_range=max_range, min_range=min_range, channel=channel, num_classes=num_classes, z_min=z_min,
                z_step=z_step, min_cell_points=min_cell_points, ignore=tuple(int(l) for l in ignore))


def cells(xyz, origin, tables, R: int, S: int, min_range: float):
    """rules 1 and 3 for float32 points (finite ones): (keep[n] bool, ring[n], sector[n], d[n, 3] float32)"""
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    o = np.zeros(3, np.float32) if origin is None else np.asarray(origin, dtype=np.float64).astype(np.float32)
    edge2, cos_half, sin_half = tables["edge2"], tables["cos_half"], tables["sin_half"]
    with np.errstate(over="ignore", invalid="ignore"):
        d = (p - o[None, :]).astype(np.float32)
        dx, dy = d[:, 0], d[:, 1]
        xx = (dx * dx).astype(np.float32)
        yy = (dy * dy).astype(np.float32)
        d2 = (xx + yy).astype(np.float32)
        D = d2.astype(np.float64)
        keep = (D < edge2[R]) & (D >= min_range * min_range)
        ring = (D[:, None] >= edge2[None, 1:R]).sum(axis=1)
        lower = ~((dy > 0) | ((dy == 0) & (dx > 0)))
        xp = np.where(lower, -dx, dx).astype(np.float64)
        yp = np.where(lower, -dy, dy).astype(np.float64)
        u = cos_half[None, 1:] * yp[:, None]
        v = sin_half[None, 1:] * xp[:, None]
        sector = ((u - v) >= 0.0).sum(axis=1) + np.where(lower, S // 2, 0)
    return keep, ring.astype(np.int64), sector.astype(np.int64), d


def describe(xyz, labels, P, tables, origin=None):
    """rules 1-4: (desc[R, S] uint8, {"n_in", "n_kept", "n_cells"}).  Points that are not finite take no part (the library never
    holds them).  Raises BadLabel as the library answers SICP_ERR_BAD_LABEL."""
    R, S = P["R"], P["S"]
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    finite = np.isfinite(p).all(axis=1)
    p = p[finite]
    keep, ring, sector, d = cells(p, origin, tables, R, S, P["min_range"])
    cell = (ring * S + sector)[keep]
    desc = np.zeros(R * S, dtype=np.uint8)
    if P["channel"] == LABEL:
        C = P["num_classes"]
        lab = np.asarray(labels, dtype=np.uint32).reshape(-1)[finite][keep].astype(np.int64)
        if (lab > C).any():
            raise BadLabel()
        part = lab != 0
        for l in P["ignore"]:
            part &= lab != l
        hist = np.zeros((R * S, C + 1), dtype=np.int64)
        np.add.at(hist, (cell[part], lab[part]), 1)
        total = hist[:, 1:].sum(axis=1)
        code = 1 + np.argmax(hist[:, 1:], axis=1)  # (the first maximum: ties to the smallest label)
        desc = np.where(total >= P["min_cell_points"], code, 0).astype(np.uint8)
        desc[total == 0] = 0
    else:
        t = (d[keep, 2].astype(np.float64) - P["z_min"]) * (1.0 / P["z_step"])
        level = np.where(t < 0, 0, np.where(t >= 254, 254, np.floor(np.where((t >= 0) & (t < 254), t, 0)))).astype(np.int64)
        count = np.zeros(R * S, dtype=np.int64)
        top = np.full(R * S, -1, dtype=np.int64)
        np.add.at(count, cell, 1)
        np.maximum.at(top, cell, level)
        desc = np.where(count >= P["min_cell_points"], 1 + top, 0).astype(np.uint8)
    info = {"n_in": int(p.shape[0]), "n_kept": int(keep.sum()), "n_cells": int((desc != 0).sum())}
    return desc.reshape(R, S), info


def counts(q, e):
    """rule 5: (match[S], either[S]) of query q against entry e (both [R, S]) at every shift"""
    q = np.asarray(q, dtype=np.uint8)
    e = np.asarray(e, dtype=np.uint8)
    S = q.shape[1]
    idx = (np.arange(S)[None, :] + np.arange(S)[:, None]) % S  # idx[s, c] = (c + s) % S
    es = e[:, idx]                                             # [R, s, c]
    qq = q[:, None, :]
    match = ((qq == es) & (qq != 0)).sum(axis=(0, 2))
    either = ((qq != 0) | (es != 0)).sum(axis=(0, 2))
    return match.astype(np.int64), either.astype(np.int64)


def fraction(match: int, either: int) -> Fraction:
    return Fraction(int(match), int(either)) if either else Fraction(0)


def best_shift(q, e):
    """(shift, match, either): the largest score, ties to the smallest shift"""
    match, either = counts(q, e)
    best = 0
    for s in range(1, len(match)):
        if fraction(match[s], either[s]) > fraction(match[best], either[best]):
            best = s
    return best, int(match[best]), int(either[best])


def key30(match: int, either: int) -> int:
    return (int(match) << 30) // int(either) if either else 0


def yaw_of(shift: int, S: int) -> float:
    return float(shift - S if 2 * shift > S else shift) * (TWO_PI / float(S))


def query(q, entries, first=0, count=-1, top_k=5, min_score=0.0):
    """rule 6: the candidates of q among entries[first : first + count], best first, as the library returns them"""
    S = np.asarray(q).shape[1]
    n = len(entries)
    if count < 0:
        count = n - first
    rows = []
    for i in range(first, first + count):
        s, m, e = best_shift(q, entries[i])
        rows.append((fraction(m, e), i, s, m, e))
    rows.sort(key=lambda r: (-r[0], r[1]))
    out = []
    for f, i, s, m, e in rows[:top_k]:
        score = float(m) / float(e) if e else 0.0
        if not score >= min_score:
            break
        out.append({"id": i, "shift": s, "match": m, "either": e, "score": score, "yaw": yaw_of(s, S)})
    return out
