"""Hand-made `Extrema` for the tests of aurora_amd.links: tables of chosen flat indices on small grids, the hand-made cases with
their answers written down, and THE RULE of aurora_amd/links.py as a plain-Python double loop over live rows."""
import math

import numpy as np
import torch

from aurora_amd import distances
from aurora_amd._sphere import EARTH_RADIUS
from aurora_amd.extrema import Extrema

INF_BITS = 0x7FF0000000000000
LAT19 = np.linspace(90, -90, 19)                 # 10 degrees a row: row 0 and row 18 are poles, row 9 is the equator (sin 0, cos 1)
LON_WRAP = np.arange(36) * 10.0                  # a full circle: column 35 is next to column 0
LON_REGIONAL = 5.0 + 9.5 * np.arange(36)         # 332.5 degrees: column 35 is 35 steps from column 0


def grid(wrap):
    return LAT19, (LON_WRAP if wrap else LON_REGIONAL), wrap


def make(points, lat, lon, wrap, max_points, count=None, device="cpu", kind="min", name="x", radius_km=300.0):
    """An `Extrema` of one surface variable with a plane per entry of `points`: a list of (row, column) pairs or of flat
    indices, in table order.  `count`: per plane, where it is not the number of points."""
    H, W = len(lat), len(lon)
    n = len(points)
    table = np.zeros((n, max_points, 2), dtype=np.int64)
    counts = np.zeros(n, dtype=np.int32)
    for p, pts in enumerate(points):
        flat = [int(q[0]) * W + int(q[1]) if isinstance(q, tuple) else int(q) for q in pts]
        counts[p] = len(flat) if count is None else count[p]
        flat = flat[:max_points]
        table[p, :len(flat), 0] = flat
        table[p, :len(flat), 1] = 0x80000000 + 1000 + np.arange(len(flat))     # keys of small positive floats
    t = lambda a: torch.from_numpy(np.asarray(a)).to(device)  # noqa: E731
    empty = torch.empty((n, 0, 0), device=device)
    return Extrema(empty.to(torch.int32), empty, t(table), t(counts), t(np.asarray(lat, dtype=np.float64)),
                   t(np.asarray(lon, dtype=np.float64)), ((name, 0, (n,)),), kind, radius_km, wrap, max_points, None)


def key_of(fa, fb, s, c, cd, W, wrap):
    """THE RULE, point 3, with Python floats: every operation is rounded on its own."""
    if fa == fb:
        return 0.0
    (ia, ja), (ib, jb) = divmod(fa, W), divmod(fb, W)
    gap = abs(ja - jb)
    if wrap:
        gap = min(gap, W - gap)
    m1 = float(s[ia]) * float(s[ib])
    m2 = float(c[ia]) * float(c[ib])
    m3 = m2 * float(cd[gap])
    a = m1 + m3
    key = 1.0 - a
    return 0.0 if key < 0.0 else key


def bits_of(key):
    return int(np.float64(key).view(np.int64))


def brute(a, b, max_km, keep_a=None, keep_b=None):
    """forward and backward of two host `Extrema` by a double loop over live rows; keep: (n_planes, M) bool arrays or None."""
    lat, lon, wrap = a.grid_lat.numpy(), a.grid_lon.numpy(), bool(a.wrap)
    s, c, cd = distances.tables_of(lat, lon, wrap)
    key_max, W = distances.key_max_of(max_km), len(lon)
    ta, tb, ca, cb = a.table_table.numpy(), b.table_table.numpy(), a.count_table.numpy(), b.count_table.numpy()
    n, ma, mb = ta.shape[0], ta.shape[1], tb.shape[1]
    forward = np.empty((n, ma, 2), dtype=np.int64)
    backward = np.empty((n, mb, 2), dtype=np.int64)
    forward[..., 0] = backward[..., 0] = INF_BITS
    forward[..., 1] = backward[..., 1] = -1
    for p in range(n):
        la = [r for r in range(min(int(ca[p]), ma)) if keep_a is None or keep_a[p, r]]
        lb = [r for r in range(min(int(cb[p]), mb)) if keep_b is None or keep_b[p, r]]
        for out, mine, tm, other, to in ((forward, la, ta, lb, tb), (backward, lb, tb, la, ta)):
            for r in mine:
                best = (math.inf, -1)
                for q in other:
                    key = key_of(int(tm[p, r, 0]), int(to[p, q, 0]), s, c, cd, W, wrap)
                    if key <= key_max and key < best[0]:
                        best = (key, q)
                if best[1] >= 0:
                    out[p, r] = bits_of(best[0]), best[1]
    return forward, backward


def random_points(rng, H, W, n):
    """n distinct flat indices in ascending order, as `extrema` writes them."""
    return np.sort(rng.choice(H * W, size=n, replace=False)).tolist()


# ---- the hand-made cases: name -> (wrap, a points, b points, kwargs of `make` for a, for b, max_km, keep_a, keep_b, the answers) ----
NONE = (INF_BITS, -1)


def hand_made():
    """name -> dict(a=, b=, max_km=, keep_a=, keep_b=, next=, prev=, nearest_next=, nearest_prev=): one plane each, 4 rows a side."""
    cases = {}

    def case(name, wrap, pa, pb, max_km, *, next, prev, nearest_next=None, nearest_prev=None, count_a=None, count_b=None,
             keep_a=None, keep_b=None, ma=4, mb=4):
        lat, lon, _ = grid(wrap)
        a = make([pa], lat, lon, wrap, ma, None if count_a is None else [count_a])
        b = make([pb], lat, lon, wrap, mb, None if count_b is None else [count_b])
        pad = lambda rows, m: list(rows) + [-1] * (m - len(rows))  # noqa: E731
        cases[name] = dict(a=a, b=b, max_km=max_km, keep_a=keep_a, keep_b=keep_b, next=pad(next, ma), prev=pad(prev, mb),
                           nearest_next=pad(next if nearest_next is None else nearest_next, ma),
                           nearest_prev=pad(prev if nearest_prev is None else nearest_prev, mb))

    # two b points at the same key (two columns either side on the equator): the smaller row wins
    case("equal keys", True, [(9, 10)], [(9, 12), (9, 8)], 3000.0, next=[0], prev=[0, -1], nearest_prev=[0, 0])
    # columns 0 and 35: one step apart across the seam (1112 km on the equator), 35 steps apart (27.5 degrees the short way) without
    case("across the seam", True, [(9, 0)], [(9, 35)], 1500.0, next=[0], prev=[0])
    case("no seam on a regional grid", False, [(9, 0)], [(9, 35)], 1500.0, next=[-1], prev=[-1])
    # a pole row is one point of the sphere: key 0 between all of its columns, so the smallest row wins
    case("pole row", True, [(0, 5), (0, 20)], [(0, 30), (0, 2), (0, 17)], 100.0, next=[0, -1], prev=[0, -1, -1],
         nearest_next=[0, 0], nearest_prev=[0, 0, 0])
    # a0 -> b0 but b0 -> a1: no link for a0
    case("triangle", True, [(9, 10), (9, 14)], [(9, 13)], 5000.0, next=[-1, 0], prev=[1], nearest_next=[0, 0])
    case("no rows in a", True, [(9, 10)], [(9, 11)], 5000.0, count_a=0, next=[-1], prev=[-1])
    case("no rows in b", True, [(9, 10)], [(9, 11)], 5000.0, count_b=0, next=[-1], prev=[-1])
    # count 7 > max_points 2: the tables are truncated, rows 0 and 1 are live on either side
    case("truncated", True, [(9, 10), (9, 20), (9, 30)], [(9, 21), (9, 11), (9, 31)], 1500.0, count_a=7, count_b=7, ma=2, mb=2,
         next=[1, 0], prev=[1, 0])
    # the nearest partner of a0 is b0; without it, b1
    case("keep removes the nearest", True, [(9, 10)], [(9, 11), (9, 12)], 5000.0, keep_b=[False, True, True, True],
         next=[1], prev=[-1, 0])
    case("keep removes a", True, [(9, 10), (9, 12)], [(9, 11)], 5000.0, keep_a=[False, True, True, True], next=[-1, 0], prev=[1])
    return cases


def exact_cases():
    """name -> dict(a=, b=, max_km=, forward=, backward=): one plane, 4 rows a side, every (key_bits, row) written down.

    "same flat index": on a row where key_of of a point and ITSELF is not 0, so that the rule, not the formula, gives the 0.
    "key at key_max" / "key above key_max": two points of the equator (s = 0, c = 1) three columns apart have key 1 - cd[3];
    max_km is chosen among the neighbouring floats of 30 degrees of arc in kilometres so that key_max_of(max_km) IS that number,
    and then so that it is the next number below it."""
    lat, lon, wrap = grid(True)
    s, c, cd = distances.tables_of(lat, lon, wrap)
    none = [INF_BITS, -1]
    rows = [i for i in range(19) if 1.0 - (float(s[i]) * float(s[i]) + (float(c[i]) * float(c[i])) * 1.0) != 0.0]
    assert rows, "no row of this grid shows the difference: the formula alone gives 0 everywhere"
    i = rows[0]
    cases = {"same flat index": dict(a=make([[(i, 7), (i, 9)]], lat, lon, wrap, 4), b=make([[(i, 8), (i, 7)]], lat, lon, wrap, 4),
                                     max_km=50.0, forward=[[0, 1], none, none, none],      # (one column away is farther than 50 km)
                                     backward=[none, [0, 0], none, none])}
    key = 1.0 - float(cd[3])
    km = math.radians(30.0) * EARTH_RADIUS / 1000.0
    ups, downs = [km], [km]
    for _ in range(64):
        ups.append(float(np.nextafter(ups[-1], np.inf)))
        downs.append(float(np.nextafter(downs[-1], -np.inf)))
    at = [x for x in ups + downs if distances.key_max_of(x) == key]
    below = [x for x in downs if distances.key_max_of(x) < key]
    assert at and below, "no float near 30 degrees of arc gives this key_max"
    pa, pb = [[(9, 10), (9, 20)]], [[(9, 13), (9, 24)]]               # a0 - b0: 3 columns, key == key_max; a1 - b1: 4 columns
    cases["key at key_max"] = dict(a=make(pa, lat, lon, wrap, 4), b=make(pb, lat, lon, wrap, 4), max_km=at[0],
                                   forward=[[bits_of(key), 0], none, none, none], backward=[[bits_of(key), 0], none, none, none])
    cases["key above key_max"] = dict(a=make(pa, lat, lon, wrap, 4), b=make(pb, lat, lon, wrap, 4), max_km=max(below),
                                      forward=[none] * 4, backward=[none] * 4)      # key_max one step smaller: out of reach
    return cases


EXACT = ("key above key_max", "key at key_max", "same flat index")
