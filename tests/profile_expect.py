"""Expected values for kh_profile* and kh_profile_records*, from the oracle only.

oracle_profile is the definition: every position is O.from_sub (is the window a k-mer) + O.canonical + the table's get, with the
quality rule min_quality.saturating_add(33).  np_profile is its vectorised numpy twin for inputs at size; check_twin holds the
twin to the primitives window by window on at least `npos` positions and returns it.  A row of kh_profile_records* is a
segment reduction of that profile, written in numpy: rows_of."""
import numpy as np

import oracle_lib as O

NO = 0xFFFFFFFF
SAT = 0xFFFFFFFE
NONE = 0xFFFFFFFF
(WINDOWS, PRESENT, IN_RANGE, MIN, MAX, SUM_LO, SUM_HI, FIRST_LOW) = range(8)


def thr_of(minq):
    return min(int(minq) + 33, 255)  # min_quality.saturating_add(33) on u8


def oracle_profile(flat, k, table, qual=None, minq=None, positions=None):
    """Entry by entry from the oracle primitives.  table: an OracleMap, or a dict key -> count."""
    flat = bytes(flat)
    n = len(flat)
    get = table.get
    out = np.full(n, NO, dtype=np.uint32)
    thr = thr_of(minq) if (qual is not None and minq is not None) else None
    q = bytes(qual) if qual is not None else None
    for i in (range(n) if positions is None else positions):
        if i + k > n:
            continue
        w = flat[i:i + k]
        norm, err = O.from_sub(w)
        if norm is None:
            continue
        if thr is not None and min(q[i:i + k]) < thr:
            continue
        key, _ = O.canonical(norm)
        c = get(key)
        out[i] = min(int(c or 0), SAT)
    return out


_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i
    _CODE[_ch + 32] = _i


def np_profile(flat, k, keys, counts, qual=None, minq=None):
    """The numpy twin (checked against oracle_profile by its users)."""
    flat = np.frombuffer(bytes(flat), dtype=np.uint8) if not isinstance(flat, np.ndarray) else flat
    n = flat.size
    out = np.full(n, NO, dtype=np.uint32)
    nw = n - k + 1
    if nw <= 0:
        return out
    code = _CODE[flat]
    bad = code == 255
    if qual is not None and minq is not None:
        bad |= np.asarray(qual, dtype=np.uint8) < thr_of(minq)
    cs = np.concatenate(([0], np.cumsum(bad, dtype=np.int64)))
    good = (cs[k:] - cs[:-k]) == 0
    c64 = (code & 3).astype(np.uint64)
    fwd = np.zeros(nw, dtype=np.uint64)
    rc = np.zeros(nw, dtype=np.uint64)
    for j in range(k):
        fwd |= c64[j:j + nw] << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - c64[j:j + nw]) << np.uint64(2 * j)
    canon = np.minimum(fwd, rc)
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint64)
    val = np.zeros(nw, dtype=np.uint64)
    if keys.size:
        pos = np.minimum(np.searchsorted(keys, canon), keys.size - 1)
        hit = keys[pos] == canon
        val[hit] = counts[pos[hit]]
    out[:nw][good] = np.minimum(val, np.uint64(SAT)).astype(np.uint32)[good]
    return out


def check_twin(flat, k, m, keys, counts, qual=None, minq=None, npos=2000, seed=1):
    n = len(flat)
    pos = np.unique(np.concatenate((np.random.default_rng(seed).integers(0, n, size=npos + 500), np.arange(min(n, 300)),
                                    np.arange(max(0, n - 300), n))))
    assert pos.size >= min(npos, n)
    want = oracle_profile(flat, k, m, qual, minq, positions=pos.tolist())
    got = np_profile(flat, k, keys, counts, qual, minq)
    assert np.array_equal(got[pos], want[pos]), "the numpy twin differs from the oracle primitives"
    return got


def rows_of(P, rec_start, lo, hi):
    """The definition of kh_profile_records*: row r = the reduction over P[rec_start[r] : rec_start[r + 1]], NO_WINDOW skipped.
    Vectorised with prefix sums / reduceat over the profile; rows_of_slow is the same record by record."""
    P = np.asarray(P, dtype=np.uint32)
    rs = np.asarray(rec_start, dtype=np.int64)
    nrec = rs.size - 1
    rows = np.zeros((nrec, 8), dtype=np.uint32)
    rows[:, FIRST_LOW] = NONE
    if nrec == 0:
        return rows
    win = P != NO
    v = np.where(win, P, 0).astype(np.uint64)
    pre = lambda a: np.concatenate((np.zeros(1, np.uint64), np.cumsum(a, dtype=np.uint64)))
    seg = lambda a: (pre(a)[rs[1:]] - pre(a)[rs[:-1]])
    windows = seg(win)
    rows[:, WINDOWS] = windows
    rows[:, PRESENT] = seg(win & (P > 0))
    rows[:, IN_RANGE] = seg(win & (P >= lo) & (P <= hi))
    s = seg(v)
    rows[:, SUM_LO] = (s & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rows[:, SUM_HI] = (s >> np.uint64(32)).astype(np.uint32)
    # min / max / first_low: reduceat over the non-empty records, cut at (start, end) pairs -- every second result is a record's
    # (one sentinel entry behind the profile makes end == n a valid cut)
    ne = np.flatnonzero(rs[1:] > rs[:-1])
    if ne.size:
        big = np.uint64(1) << np.uint64(40)
        idx = np.arange(P.size, dtype=np.uint64)
        cuts = np.stack((rs[:-1][ne], rs[1:][ne]), axis=1).reshape(-1)
        red = lambda arr, op: op.reduceat(np.concatenate((arr, np.zeros(1, np.uint64))), cuts)[::2]
        mn = red(np.where(win, P.astype(np.uint64), big), np.minimum)
        mx = red(v, np.maximum)
        fl = red(np.where(win & (P < lo), idx, big), np.minimum)
        has = windows[ne] > 0
        rows[ne, MIN] = np.where(has, mn, np.uint64(0)).astype(np.uint32)
        rows[ne, MAX] = mx.astype(np.uint32)
        rows[ne, FIRST_LOW] = np.where(fl < big, fl - rs[:-1][ne].astype(np.uint64), np.uint64(NONE)).astype(np.uint32)
    return rows


def rows_of_slow(P, rec_start, lo, hi):
    """rows_of record by record in plain Python (what the vectorised form is held to on small inputs)."""
    nrec = len(rec_start) - 1
    rows = np.zeros((nrec, 8), dtype=np.uint32)
    for r in range(nrec):
        seg = [int(x) for x in P[int(rec_start[r]):int(rec_start[r + 1])]]
        vals = [(i, x) for i, x in enumerate(seg) if x != NO]
        s = sum(x for _, x in vals)
        low = [i for i, x in vals if x < lo]
        rows[r] = [len(vals), sum(x > 0 for _, x in vals), sum(lo <= x <= hi for _, x in vals),
                   min((x for _, x in vals), default=0), max((x for _, x in vals), default=0), s & 0xFFFFFFFF, s >> 32,
                   low[0] if low else NONE]
    return rows


def starts_of(flat):
    """rec_start of a flat '\\n'-separated buffer: the start byte of every record, and n (an unterminated last run is a record)."""
    flat = np.asarray(flat, dtype=np.uint8)
    nl = np.flatnonzero(flat == 10)
    starts = np.concatenate(([0], nl + 1))
    if starts[-1] == flat.size:
        starts = starts[:-1]
    return np.concatenate((starts, [flat.size])).astype(np.uint64)
