"""Planted inputs for the forward FGINN matcher (csrc/match.hip): decision boundaries, the ends of the integer ranges, and chosen
positions of the two nearest trains inside the tiles and train splits of pass 1.  Pure numpy; nothing here calls the library.

Every builder returns a list of searches (q, t, params, expect): params = the keyword arguments of match_fginn, and expect holds what
is known BY CONSTRUCTION, so that a mistake shared by the kernel and a reference still fails:
  case      name of the search
  names     one label per query
  t         per query: the planted nearest train, REJECTED (no tentative) or UNKNOWN
  t_bad     per query: the planted train the tentative must name as t_bad, or UNKNOWN
  planted   [(query, train, squared distance)] the builder claims
  grid      (tile_positions, many_candidates) the pass-1 geometry the list lengths are meant to reach

Distances are laid out as sums of a few squares: a train at distance d from a query differs from it by v1, v2, ... in a few
descriptor elements, v1^2 + v2^2 + ... = d.  Several (query, trains) groups share one search where they can be kept apart: group g
owns a block of elements that are 255 in its query and trains and 0 elsewhere, so every train of another group is further than any
planted one."""
import numpy as np

import match_ref as ref

REGION_DTYPE = np.dtype([("x", "f8"), ("y", "f8"), ("s", "f8"), ("a11", "f8"), ("a12", "f8"), ("a21", "f8"),
                         ("a22", "f8"), ("response", "f8"), ("sub_type", "i4"), ("id", "i4"), ("parent", "i4"),
                         ("pad", "i4"), ("desc", "u1", (128,))])
REJECTED, UNKNOWN = -1, -2
FAR = 500.0                       # px: further than every contradDist used here but 1e9
FIX_MAXC = 32                     # csrc/match.hip: candidate half tiles the exact finish of pass 1 lists per query
TILE = 32                         # train rows per tile


def regions(n):
    r = np.zeros(n, REGION_DTYPE)
    r["s"] = 2.0; r["a11"] = 1.0; r["a22"] = 1.0
    return r


def random_regions(n, rng, extent=4000.0):
    """uniform descriptor bytes (two of them are ~1.4e6 apart, none closer than ~6e5) at float32 coordinates"""
    r = regions(n)
    r["x"] = rng.uniform(0, extent, n).astype(np.float32)
    r["y"] = rng.uniform(0, extent, n).astype(np.float32)
    r["desc"] = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    return r


def squares(d, cap=255):
    """d as a sum of squares of integers <= cap, largest first"""
    out = []
    while d > 0:
        v = min(cap, int(np.sqrt(d)))
        while v * v > d:
            v -= 1
        out.append(v); d -= v * v
    return out


def plant(base, d, start=0):
    """a copy of the descriptor `base` at squared distance d from it: elements start, start + 1, ... move by the squares of d, up where
    that stays within a byte and down otherwise"""
    out = np.asarray(base, np.int64).copy()
    for n, v in enumerate(squares(d)):
        e = start + n
        assert e < 128
        out[e] += v if out[e] + v <= 255 else -v
        assert 0 <= out[e] <= 255
    return out.astype(np.uint8)


def _expect(case, names):
    n = len(names)
    return {"case": case, "names": list(names), "t": np.full(n, UNKNOWN), "t_bad": np.full(n, UNKNOWN), "planted": []}


def check_expectations(tent, case):
    """the construction-time expectations of a search on a tentative list (the reference's here, the library's in the GPU suite)"""
    q, t, params, ex = case
    name = ex["case"]
    row = {int(qi): k for k, qi in enumerate(tent["q"])}
    assert len(row) == len(tent), (name, "a query twice")
    if ex.get("all"):
        assert len(tent) == len(q), (name, "accepted", len(tent), "of", len(q))
    for qi in range(len(q)):
        want_t, want_bad = int(ex["t"][qi]), int(ex["t_bad"][qi])
        label = (name, ex["names"][qi])
        if want_t == REJECTED:
            assert qi not in row, label + ("emitted, planted as rejected", tent[row[qi]] if qi in row else None)
        elif want_t != UNKNOWN:
            assert qi in row, label + ("rejected, planted as accepted",)
            assert int(tent["t"][row[qi]]) == want_t, label + ("t", int(tent["t"][row[qi]]), want_t)
            if want_bad != UNKNOWN:
                assert int(tent["t_bad"][row[qi]]) == want_bad, label + ("t_bad", int(tent["t_bad"][row[qi]]), want_bad)


def pack_groups(case, groups, params, copies=1):
    """One search of len(groups) queries (each `copies` times, at different places).  A group is {name, trains: [(d, dx, dy[, ulps])],
    outcome: None (rejected) or (nearest, t_bad) as positions in its train list}: train 0 sits at the group's own place, the others
    dx, dy from it (small integers: the sums are exact in float32), x moved by `ulps` float32 steps.  Returns None when the groups
    cannot be kept apart in 128 elements."""
    G = len(groups)
    P = max(len(squares(tr[0])) for g in groups for tr in g["trains"])
    dmax = max(tr[0] for g in groups for tr in g["trains"])
    B = (128 - P) // G if G > 1 else 0
    if P > 128 or (G > 1 and 2 * B * 255 * 255 <= dmax):
        return None
    n_t = sum(len(g["trains"]) for g in groups)
    q, t = regions(G * copies), regions(n_t)
    ex = _expect(case, ["%s #%d" % (g["name"], c) for g in groups for c in range(copies)])
    ti = 0
    for gi, g in enumerate(groups):
        base = np.zeros(128, np.int64)
        base[:P] = 255 * (gi & 1)                   # the planted differences go down from 255 in odd groups, up from 0 in even ones
        base[P + gi * B: P + (gi + 1) * B] = 255
        x0, y0 = 64.0 + 40.0 * gi, 96.0 + 8.0 * gi          # (exact in float32, as are the offsets added to them)
        for c in range(copies):
            qi = gi * copies + c
            q["desc"][qi] = base
            q["x"][qi], q["y"][qi] = 10.0 + 3.0 * qi, 700.0 + 90.0 * c
            if g["outcome"] is None:
                ex["t"][qi] = REJECTED
            else:
                ex["t"][qi], ex["t_bad"][qi] = ti + g["outcome"][0], ti + g["outcome"][1]
            for k, tr in enumerate(g["trains"]):
                ex["planted"].append((qi, ti + k, tr[0]))
        for tr in g["trains"]:
            t["desc"][ti] = plant(base, tr[0])
            x = np.float32(x0 + tr[1])
            for _ in range(abs(tr[3]) if len(tr) > 3 else 0):
                x = np.nextafter(x, np.float32(np.inf if tr[3] > 0 else -np.inf))
            t["x"][ti], t["y"][ti] = x, np.float32(y0 + tr[2])
            ti += 1
    return q, t, dict(params), ex


def _pack_or_split(case, groups, params):
    """the groups in one search, or - where 128 elements cannot keep them apart - every group in a search of its own"""
    one = pack_groups(case, groups, params)
    if one is not None:
        return [one]
    return [pack_groups("%s, %s" % (case, g["name"]), [g], params) for g in groups]


# ---- the ratio test: fl32(d0 / d) <= ratio^2 --------------------------------------------------------------------------------------
RATIOS = (0.5, 0.8, 0.95, 0.999)          # 0.25 is a float; 0.64, 0.9025 and 0.998001 are not
RATIO_D0 = (1, 3, 100, (1 << 20) + 1)


def rounding_d0(ratio):
    """the first d0 above 2^20 whose D* is not ceil(d0 / ratio^2): the float32 rounding of the quotient moves the boundary there
    (1 048 668 for 0.95, 1 048 925 for 0.999; ratios 0.5 and 0.8 have none)"""
    sq = np.float64(ratio) * np.float64(ratio)
    for d0 in range((1 << 20) + 2, (1 << 20) + 2000):
        if ref.dstar(d0, ratio) != int(np.ceil(d0 / sq)):
            return d0
    return None


def ratio_boundary():
    """For every ratio and d0: the runner-up at D* - 1, D* and D* + 1 (D* = the smallest d with fl32(d0 / d) <= ratio^2), 5 px or 500 px
    from the nearest train, and a third train well above D*, far away.
      D* - 1 near   fails the ratio test, is consistent: the walk goes on and emits the third train (t_bad = third)
      D* - 1 far    fails, contradicts: rejected
      D*, D* + 1    passes: t_bad = the runner-up wherever it lies (the ratio test comes first)
    d0 = 1, 3, 100, 2^20 + 1 and, where the ratio has one, the first d0 above 2^20 at which float32 rounding moves D* off ceil(d0 / ratio^2);
    and d0 = 0 with a second train at distance 0: 0 / 0 is NaN and does not pass, the walk goes on or stops on geometry."""
    out = []
    for ratio in RATIOS:
        params = {"ratio": ratio, "contrad": 10.0, "nn": 50}
        for d0 in RATIO_D0 + ((rounding_d0(ratio),) if rounding_d0(ratio) else ()):
            D = ref.dstar(d0, ratio)
            groups = []
            for off in (-1, 0, 1):
                for near in (True, False):
                    runner = (D + off, 3.0, 4.0) if near else (D + off, 0.0, FAR)
                    outcome = (0, 1) if off >= 0 else ((0, 2) if near else None)
                    groups.append({"name": "runner-up at D*%+d = %d %s" % (off, D + off, "near" if near else "far"),
                                   "trains": [(d0, 0.0, 0.0), runner, (D + 10001, 300.0, -40.0)], "outcome": outcome})
            out += _pack_or_split("ratio_boundary ratio=%g d0=%d" % (ratio, d0), groups, params)
        groups = [{"name": "duplicate at distance 0 %s" % ("near" if near else "far"),
                   "trains": [(0, 0.0, 0.0), (0, 3.0, 4.0) if near else (0, 0.0, FAR), (77, 300.0, -40.0)],
                   "outcome": (0, 2) if near else None} for near in (True, False)]
        out += _pack_or_split("ratio_boundary ratio=%g d0=0" % ratio, groups, params)
    return out


# ---- the contradiction test: dist^2 > contradDist^2, strict -----------------------------------------------------------------------
def contrad_boundary():
    """d0 = 100, ratio 0.8 (D* = 157).  A neighbour below D* sits at exactly contradDist from the nearest train ((3, 4) with 5, (6, 8) with
    10, to either side) - consistent, the walk reaches the train planted at D* - or one float32 ulp further in x - contradicting, the
    query is rejected.  The neighbour is the second, third or fifth of the walk (the second is decided by match_mid_kernel, the others in
    pass 2); the neighbours before it lie 1 px from the nearest train.  "One ulp" is a step of the train's float32 x coordinate."""
    out = []
    d0, ratio = 100, 0.8
    D = ref.dstar(d0, ratio)
    assert D == 157
    for (ox, oy), cd in (((3.0, 4.0), 5.0), ((6.0, 8.0), 10.0)):
        groups = []
        for pos in (1, 2, 4):
            for sign in (1.0, -1.0):
                for further in (False, True):
                    trains = [(d0, 0.0, 0.0)] + [(d0 + 1 + k, 1.0, 0.0) for k in range(pos - 1)]
                    trains += [(d0 + 10, sign * ox, oy, int(sign) if further else 0), (D, 0.0, FAR)]
                    groups.append({"name": "walk position %d at %s(%g, %g)%s" % (pos + 1, "-" if sign < 0 else "+", ox, oy, " + 1 ulp" if further else ""),
                                   "trains": trains, "outcome": None if further else (0, len(trains) - 1)})
        out += _pack_or_split("contrad_boundary contradDist=%g" % cd, groups, {"ratio": ratio, "contrad": cd, "nn": 50})
    return out


# ---- the nn cap -------------------------------------------------------------------------------------------------------------------
NN_CAP_C = (0, 1, 2, 3, 4, 6)
NN_CAP_NN = (1, 2, 3, 4, 5, 6, 7, 8, 9, 50)       # 1, 2, 3, 50 and c + 1, c + 2, c + 3 of every c above


def nn_cap():
    """A query with c consistent trains below D* and then one above it is accepted from nn = c + 2 on (the walk visits K - 1 = nn - 1
    neighbours; the one above D* is neighbour c + 1).  One search per nn with a group for every c.  And lists shorter than nn:
    c + 1 trains, all below D* - nothing is emitted - and c + 2 trains, the last one above D* - emitted, the count below D* is K - 2."""
    out = []
    d0, ratio = 100, 0.8
    D = ref.dstar(d0, ratio)

    def below(c):
        return [(d0, 0.0, 0.0)] + [(d0 + 1 + k, 1.0, float(k)) for k in range(c)]
    for nn in NN_CAP_NN:
        groups = [{"name": "c=%d" % c, "trains": below(c) + [(D + 1, 0.0, FAR), (D + 500, FAR, 0.0)],
                   "outcome": (0, c + 1) if nn >= c + 2 else None} for c in NN_CAP_C]
        out += _pack_or_split("nn_cap nn=%d" % nn, groups, {"ratio": ratio, "contrad": 10.0, "nn": nn})
    for c in (1, 2, 3):
        for with_above in (False, True):
            g = {"name": "c=%d" % c, "trains": below(c) + ([(D, 0.0, FAR)] if with_above else []), "outcome": (0, c + 1) if with_above else None}
            for nn in (50, len(g["trains"])):                      # n_t < nn and n_t == nn
                out.append(pack_groups("nn_cap n_t=%d nn=%d" % (len(g["trains"]), nn), [g], {"ratio": ratio, "contrad": 10.0, "nn": nn}, copies=3))
    return out


# ---- the ends of the integer ranges -----------------------------------------------------------------------------------------------
def _extreme_rows():
    """(descriptors, kind per row): the six extreme descriptors, then single-element changes of each (odd norms among them)"""
    half = np.r_[np.zeros(64, np.int64), np.full(64, 255)]
    base = [np.zeros(128, np.int64), np.full(128, 255), half, half[::-1].copy(), np.full(128, 127), np.full(128, 128)]
    rows, kind = list(base), list(range(6))
    for k in range(27):
        b = base[k % 6].copy()
        e = (11 * k + 5) % 128
        step = 1 + k // 12                         # by 1, later by 2 and 3
        b[e] += step if b[e] < 128 else -step
        rows.append(b); kind.append(-1)
    return np.array(rows, np.uint8), kind


# squared distances between the six extreme descriptors, worked out by hand: 128 * 255^2, 64 * 255^2, 128 * 127^2, 128 * 128^2,
# 64 * 127^2 + 64 * 128^2, 128 * 1
_E = {(0, 1): 8323200, (0, 2): 4161600, (0, 3): 4161600, (0, 4): 2064512, (0, 5): 2097152, (1, 2): 4161600, (1, 3): 4161600,
      (1, 4): 2097152, (1, 5): 2064512, (2, 3): 8323200, (2, 4): 2080832, (2, 5): 2080832, (3, 4): 2080832, (3, 5): 2080832, (4, 5): 128}


def extremes():
    """Queries and trains that are all 0, all 255, half and half, all 127, all 128, and single-element changes of these: the largest and
    smallest dot products and norms the accumulator seeds meet, the maximum distance 128 * 255^2 included.  Train lists of 1, 5 and 33
    rows leave padded rows in the last tile."""
    rows, kind = _extreme_rows()
    out = []
    order = {1: [1], 5: [1, 0, 2, 4, 5], 33: list(range(33))}
    qsel = [0, 1, 2, 3, 4, 5] + list(range(6, 18))
    for n_t, tsel in order.items():
        for ratio, cd in ((0.8, 10.0), (0.999, 1e9)):
            q, t = regions(len(qsel)), regions(n_t)
            q["desc"], t["desc"] = rows[qsel], rows[tsel]
            q["x"] = 20.0 * np.arange(len(q)); q["y"] = 50.0
            t["x"] = 7.0 * (np.arange(n_t) % 6); t["y"] = 9.0 * (np.arange(n_t) // 6)
            ex = _expect("extremes n_t=%d ratio=%g contradDist=%g" % (n_t, ratio, cd), ["query row %d" % r for r in qsel])
            for qi, qr in enumerate(qsel):
                for ti, tr in enumerate(tsel):
                    a, b = kind[qr], kind[tr]
                    if a >= 0 and b >= 0:
                        ex["planted"].append((qi, ti, 0 if a == b else _E[(min(a, b), max(a, b))]))
                if n_t == 1:
                    ex["t"][qi] = REJECTED                 # a single train: no neighbour to compare with
                elif qr in tsel:
                    ex["t"][qi] = tsel.index(qr)           # its twin at distance 0; the quotient 0 passes at the next train
            out.append((q, t, {"ratio": ratio, "contrad": cd, "nn": 50}, ex))
    return out


# ---- positions inside the tiles and train splits of pass 1 -------------------------------------------------------------------------
TILE_POSITION_TPS = (1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15)
PLACEMENTS = ("same half tile", "two halves of one tile", "first and last tile of a split", "rows 0 and 31 of a tile",
              "last rows of the last, partial tile", "first and last split", "tie across two splits")


def tile_positions_size(tps, short):
    """(n_t, n_tiles, splits) of a 70-query search meant to run `tps` tiles per train split: 256 full splits, or (short) 248 / 253
    splits of which the last holds fewer tiles (tps = 1 has no short split: 253 splits); the last tile holds 21 rows"""
    if not short:
        n_tiles = 256 * tps
    elif tps == 1:
        n_tiles = 253
    else:
        n_tiles = (247 if tps % 2 == 0 else 252) * tps + max(1, tps // 2)
    return TILE * n_tiles - 11, n_tiles, -(-n_tiles // tps)


def tile_positions(tps, short):
    """70 random queries against random trains (far from everything), and for query i planted trains: the nearest at d0 = 50 + i and the
    runner-up at one of PLACEMENTS[i % 7]; by i % 3
      0  the runner-up and two or three more trains in other tiles and splits lie below D*, near the nearest train: pass 2 counts them
         and the query is accepted with the train planted at D* or D* + 1 (far away) as t_bad
      1  the runner-up lies at D* or D* + 1: accepted, t_bad = the runner-up (a tie cannot: one train at D* follows it)
      2  the runner-up lies at D* - 1 (a tie: at d0), far from the nearest: rejected."""
    ratio = 0.8
    n_t, n_tiles, splits = tile_positions_size(tps, short)
    rng = np.random.default_rng(5000 + 2 * tps + int(short))
    q, t = random_regions(70, rng), random_regions(n_t, rng)
    ex = _expect("tile_positions tps=%d %s" % (tps, "short last split" if short else "full splits"), [""] * 70)
    ex["grid"] = {"tps": tps, "splits": splits, "n_tiles": n_tiles}
    last_start = (splits - 1) * tps
    last_len = n_tiles - last_start
    used = set()

    def take(tile, row):
        assert 0 <= tile < n_tiles
        for _ in range(TILE):
            if (tile, row) not in used and tile * TILE + row < n_t:
                used.add((tile, row))
                return tile * TILE + row
            row = (row + 1) % TILE
        raise AssertionError("tile %d is full" % tile)

    def put(i, idx, d, start, dx, dy, x0, y0):
        t["desc"][idx] = plant(q["desc"][i], d, start)
        t["x"][idx], t["y"][idx] = np.float32(x0 + dx), np.float32(y0 + dy)
        ex["planted"].append((i, idx, d))

    n4 = 0
    for i in range(70):
        p, kind = i % 7, i % 3
        d0 = 50 + i
        D = ref.dstar(d0, ratio)
        h = 3 + 3 * i                                  # a split of this query's own; h + 1 and h + 2 are nobody's
        ht = h * tps + i % tps
        if p == 0:
            a, b = take(ht, 1), take(ht, 9)
        elif p == 1:
            a, b = take(ht, 2), take(ht, 6)
        elif p == 2:
            a, b = take(h * tps, 5), take(h * tps + tps - 1, 17)
        elif p == 3:
            a, b = take(ht, 0), take(ht, 31)
        elif p == 4:
            a, b = n_t - 1 - n4, take(ht, 12)          # the last row of the list for the first such query, the rows before it for the others
            assert (n_tiles - 1, a % TILE) not in used
            used.add((n_tiles - 1, a % TILE))
            n4 += 1
        elif p == 5:
            a, b = take(i % tps, 3), take(last_start + i % last_len, 0)
        else:
            a, b = take(ht, 20), take((h + 1) * tps + i % tps, 7)
        if p in (4, 5) and (i // 7) % 2:
            a, b = b, a                                # the nearest and the runner-up change places
        x0, y0 = 100.0 + 50.0 * (i % 10), 100.0 + 50.0 * (i // 10)
        tie = p == 6
        ex["names"][i] = "query %d (%s, kind %d): nearest %d, runner-up %d" % (i, PLACEMENTS[p], kind, a, b)
        put(i, a, d0, 0, 0.0, 0.0, x0, y0)
        if kind == 2:
            put(i, b, d0 if tie else D - 1, 8, 0.0, FAR, x0, y0)
            ex["t"][i] = REJECTED
            continue
        if kind == 1 and not tie:
            put(i, b, D + i % 2, 8, *((3.0, 4.0) if i % 2 else (0.0, FAR)), x0, y0)
            ex["t"][i], ex["t_bad"][i] = a, b
            continue
        put(i, b, d0 if tie else d0 + 2, 8, 3.0, 4.0, x0, y0)
        if kind == 0:
            for e in range(2 + i % 2):
                s = ((h + 1, h + 2, h + 97)[e]) % splits
                idx = take(min(s * tps + (i + e) % tps, n_tiles - 1), (5 * e + i) % TILE)
                put(i, idx, d0 + (5, 9, 14)[e], 16 + 8 * e, -3.0, 1.0 + e, x0, y0)
        bad = take((h + 2) * tps + (i + 3) % tps, 11)
        put(i, bad, D + i % 2, 48, FAR, 0.0, x0, y0)
        ex["t"][i], ex["t_bad"][i] = a, bad
    return q, t, {"ratio": ratio, "contrad": 10.0, "nn": 50}, ex


# ---- more candidate half tiles than the exact finish of pass 1 lists ---------------------------------------------------------------
def many_candidates():
    """80 tiles, three queries: one tile per train split.  The nearest train of a query (d0 = 100) lies in split 70 + its number, and 31,
    32 or 33 trains in as many other splits tie for runner-up at 200 (above D* = 157; equal distances make equal accumulator levels):
    FIX_MAXC = 32 candidate half tiles exactly - the candidate path - and 33 and 34, which overflow the list and take the rescan over
    all trains.  The nearest train comes last in split order, the tie goes to the lowest index."""
    rng = np.random.default_rng(909)
    n_tiles = 80
    n_t = TILE * n_tiles - 5
    q, t = random_regions(3, rng), random_regions(n_t, rng)
    ex = _expect("many_candidates", ["%d candidate half tiles" % (n + 1) for n in (31, 32, 33)])
    ex["grid"] = {"tps": 1, "splits": n_tiles, "n_tiles": n_tiles}
    for i, ties in enumerate((FIX_MAXC - 1, FIX_MAXC, FIX_MAXC + 1)):
        first = None
        for j in range(ties):
            idx = (2 * j + 1 + (i == 1)) * TILE + (5 * j + 9 * i) % TILE
            first = idx if first is None else first
            t["desc"][idx] = plant(q["desc"][i], 200, (3 * j) % 100)
            t["x"][idx], t["y"][idx] = 900.0 + j, 40.0 * i
            ex["planted"].append((i, idx, 200))
        a = (70 + i) * TILE + 13 + i
        t["desc"][a] = plant(q["desc"][i], 100, 110)
        t["x"][a], t["y"][a] = 30.0, 40.0 * i
        ex["planted"].append((i, a, 100))
        ex["t"][i], ex["t_bad"][i] = a, first
    return [(q, t, {"ratio": 0.8, "contrad": 10.0, "nn": 50}, ex)]


# ---- the emit stage's block edges --------------------------------------------------------------------------------------------------
EMIT_NQ = (255, 256, 257, 511, 512, 513)


def emit_edges():
    """Every query accepted (40 random trains, ratio 0.999, no contradiction cut: some neighbour passes) and none accepted (every train
    twice, the copies far apart: the runner-up ties with the nearest and contradicts it) around the 256 queries of an emit block."""
    out = []
    for n_q in EMIT_NQ:
        rng = np.random.default_rng(n_q)
        q, t = random_regions(n_q, rng), random_regions(40, rng)
        ex = _expect("emit_edges n_q=%d all accepted" % n_q, ["query %d" % i for i in range(n_q)])
        ex["all"] = True
        out.append((q, t, {"ratio": 0.999, "contrad": 1e9, "nn": 50}, ex))
        t2 = t.copy()
        t2["desc"][20:] = t2["desc"][:20]
        t2["x"][20:] = t2["x"][:20] + FAR
        ex = _expect("emit_edges n_q=%d none accepted" % n_q, ["query %d" % i for i in range(n_q)])
        ex["t"][:] = REJECTED
        out.append((q, t2, {"ratio": 0.8, "contrad": 10.0, "nn": 50}, ex))
    return out


def small_cases():
    """every search but the tile_positions ones (which are built one at a time: up to 122 867 trains each)"""
    return ratio_boundary() + contrad_boundary() + nn_cap() + extremes() + many_candidates() + emit_edges()


def large_filler():
    """a random search that leaves 40 000 rows behind the end of whatever list follows it on the same context"""
    rng = np.random.default_rng(31337)
    return random_regions(2000, rng), random_regions(40000, rng)
