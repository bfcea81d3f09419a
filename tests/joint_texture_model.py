"""NumPy float64 definition of the table gather and its adjoint (read_gather_forward_tables / read_gather_backward_tables), and the case
set the CPU and GPU tests share.

Table t of S serves the merged ids [base_t, base_t + n_t); base_0 = 0, bases ascend, ranges do not overlap, gaps may remain.
    select      t = the last table whose base is <= id (table 0 for an id below base_1, negative ids included);
                local = clamp(id - base_t, 0, n_t - 1): an id below 0 -> row 0 of table 0, an id in a gap or past the end -> the last row
                of the last table whose base is <= id
    forward     y[p] = act_t(rows_t[local])
    adjoint     g[p] = d[p] * act_t'(y[p]),  act' = 1 (none), y (1 - y) (sigmoid), 1 - y y (tanh)
    pairs mode  g per pixel;  dense mode  drows_t[local] += g[p], a frozen table receives nothing.
With equal activations and contiguous ranges this is the plain gather over the concatenated table and its adjoint."""
import numpy as np

ACT = {"none": 0, "sigmoid": 1, "tanh": 2}
U = 2.0 ** -24


def select(ids, bases, sizes):
    """ids (...,) int -> (table (...,), local row (...,)) under the forward's clamp rules."""
    ids = np.asarray(ids, np.int64)
    bases, sizes = np.asarray(bases, np.int64), np.asarray(sizes, np.int64)
    t = np.clip(np.searchsorted(bases, ids, side="right") - 1, 0, len(bases) - 1)
    local = np.clip(ids - bases[t], 0, sizes[t] - 1)
    return t, local


def act_apply(x, act):
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    return np.tanh(x) if act == "tanh" else x


def act_slope(y, act):
    if act == "sigmoid":
        return y * (1.0 - y)
    return 1.0 - y * y if act == "tanh" else np.ones_like(y)


def forward(ids, tables, bases, acts):
    """ids (P,), tables [(n_t, C) ...] -> y (P, C) float64."""
    t, local = select(ids, bases, [len(r) for r in tables])
    y = np.empty((len(ids), tables[0].shape[1]), np.float64)
    for s, (rows, act) in enumerate(zip(tables, acts)):
        m = t == s
        y[m] = act_apply(rows.astype(np.float64)[local[m]], act)
    return y


def adjoint_pairs(ids, d, y, bases, sizes, acts):
    """d, y (P, C) -> g (P, C) float64: the gradient with respect to the raw row each pixel read."""
    t, _ = select(ids, bases, sizes)
    g = np.array(d, np.float64)
    y = None if y is None else np.asarray(y, np.float64)
    for s, act in enumerate(acts):
        if act != "none":
            m = t == s
            g[m] = g[m] * act_slope(y[m], act)
    return g


def adjoint_dense(ids, d, y, bases, sizes, acts, frozen=()):
    """-> (drows [(n_t, C) float64 | None for a frozen table], hits [(n_t,) pixels per row], mass [(n_t, C) sum of |d| per row element])."""
    t, local = select(ids, bases, sizes)
    g = adjoint_pairs(ids, d, y, bases, sizes, acts)
    Cc = g.shape[1]
    drows, hits, mass = [], [], []
    for s, n in enumerate(sizes):
        m = t == s
        acc, ab = np.zeros((n, Cc)), np.zeros((n, Cc))
        np.add.at(acc, local[m], g[m])
        np.add.at(ab, local[m], np.abs(np.asarray(d, np.float64)[m]))
        drows.append(None if s in frozen else acc)
        hits.append(np.bincount(local[m], minlength=n))
        mass.append(ab)
    return drows, hits, mass


# ---- the case set -------------------------------------------------------------------------------------------------------------------
SIZES = (5, 1, 7)
LAYOUTS = {"contiguous": (0, 5, 6), "gapped": (0, 8, 20)}
ACTS = {"mixed": ("none", "sigmoid", "tanh"), "none": ("none", "none", "none")}
LEVEL_SHAPES = ((2, 8, 6), (2, 4, 3))          # (B, h, w) of the two levels
HOT_HITS = 9


def required_ids(bases, sizes=SIZES):
    """The ids every level must contain: -3, 0, every base_t - 1, base_t and base_t + n_t - 1, an id inside a gap (where the layout has
    one), an id past the last range."""
    need = [-3, 0]
    for t, (b, n) in enumerate(zip(bases, sizes)):
        need += [b - 1] * (t > 0) + [b, b + n - 1]
    gaps = [bases[t] + sizes[t] for t in range(len(bases) - 1) if bases[t] + sizes[t] < bases[t + 1]]
    need += gaps[:1] + [bases[-1] + sizes[-1] + 2]
    return sorted(set(need))


def draw_ids(bases, rng, sizes=SIZES):
    """One int32 map per level of LEVEL_SHAPES: the required ids, one row (the second of table 2) hit by HOT_HITS pixels, random ids in
    [-1, end + 1] elsewhere, shuffled."""
    end = bases[-1] + sizes[-1]
    out = []
    for shape in LEVEL_SHAPES:
        P = int(np.prod(shape))
        fixed = required_ids(bases, sizes) + [bases[2] + 1] * HOT_HITS
        assert len(fixed) <= P
        ids = np.concatenate([fixed, rng.integers(-1, end + 2, P - len(fixed))])
        out.append(rng.permutation(ids).astype(np.int32).reshape(shape))
    return out


def cases():
    return [(Cc, layout, acts) for Cc in (4, 8) for layout in LAYOUTS for acts in ACTS]
