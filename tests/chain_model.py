"""CPU model of the chain groups of the general sorter's doubling rounds (csrc/bwt_sa.hip, k_chain_* and the chain branch of
k_sa_fill_rank2) -- test infrastructure, never imported by the product.

The schedule of sa_build_general, in plain numpy: the first rank pass at depth 5 (or at the resume depth SS_TOL_CAP, where the
doubling starts at once; or with the text rounds skipped, as sorter 2 does); text-refinement rounds add 3 to the depth until
the "deep" switch (round 1 with more than a quarter of the suffixes live, or after 3 text rounds); then prefix doubling.  A
group at depth h is the full class of suffixes that agree in their first h symbols (a suffix shorter than h is a class of its
own); singletons are resolved.

In every doubling round that the attempt schedule allows (at least `chain_min` live suffixes, bit r of `round_mask` for
doubling round r, and past round 0 only while half of the block is live) every group is put through the kernels' rule:

  candidate     min and max member, L members, d = (max - min) / (L - 1) where that divides and d <= CHAIN_DMAX  (k_chain_decide)
  verification  every member v lies on the lattice min + k d, and T[v .. v + d) == T[v + d .. v + 2 d) where v + 2 d <= max
                (so an L = 2 group is judged by the direction alone)                                         (k_chain_verify)
  direction     suffix(max) against suffix(max - d), symbol by symbol from h & ~15 on, in 16-symbol steps while the step's
                start is at most h + d + 16; where suffix(max) ends first it is the smaller; no difference: not a chain  (k_chain_dir)
  rank 2        a chain member's place in the chain, reversed where suffix(max) < suffix(max - d), replaces rank(i + h)
                                                                                                             (k_sa_fill_rank2)

`mutant` switches one part of the rule off or changes it, so that a test can show that the corpus tells it from the faithful
rule: "lattice" drops the lattice check, "u" drops the u-equality check, "u_short" stops that check one pair early
(v + 2 d < max), "direction" inverts the direction.

ADVERSARIAL: corpus blocks (mosaic(seed)) on which a mutant's suffix array is wrong, found with this model; the GPU tests run
them through the kernels with a chain attempt in every round."""
import numpy as np

CHAIN_DMAX = 4096
CHAIN_MIN = 16384           # default minimum of live suffixes per call for an attempt
CHAIN_ROUNDS = 0x15         # default round mask: doubling rounds 0, 2, 4
SS_TOL_CAP = 64             # depth the doubling resumes from after the sample sorter's tolerant form
ALL_ROUNDS = 0x7FFFFFFF     # glcPlanSetChains' every-round mask
MUTANTS = ("lattice", "u", "u_short", "direction")


class Result:
    __slots__ = ("sa", "taken", "refused", "rounds", "attempts")

    def __init__(self, sa, taken, refused, rounds, attempts):
        self.sa, self.taken, self.refused, self.rounds, self.attempts = sa, taken, refused, rounds, attempts


def _dense(k1, k2, n):
    """(order, rank) of the suffixes sorted by (k1, k2), both in [0, n]; rank = SA slot of the group head + 1"""
    key = k1 * (n + 1) + k2
    order = np.argsort(key)                                            # (the order inside a tie does not matter)
    ks = key[order]
    head = np.ones(n, dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    r = np.maximum.accumulate(np.where(head, np.arange(n), 0)) + 1
    rk = np.empty(n, dtype=np.int64)
    rk[order] = r
    return order, rk


def _shift(rk, a, n):
    """rank(i + a), 0 past the end (the shorter suffix is the smaller)"""
    out = np.zeros(n, dtype=np.int64)
    if a < n:
        out[: n - a] = rk[a:]
    return out


class prefix_ranks:
    """exact ranks of the suffixes on their first h symbols, any h"""

    def __init__(self, data):
        T = as_text(data)
        self.n = len(T)
        self.memo = {1: _dense(np.zeros(self.n, dtype=np.int64), T.astype(np.int64), self.n)[1]}

    def at(self, h):
        if h not in self.memo:
            a = h - 3 if h > 6 and h - 3 in self.memo else (h + 1) // 2      # (text rounds: 3 symbols more)
            self.memo[h] = _dense(self.at(a), _shift(self.at(h - a), a, self.n), self.n)[1]
        return self.memo[h]


def _direction(Tb, n, A, B, h, d):
    """k_chain_dir: True where suffix(A) < suffix(B), False where greater, None where no difference was found (Tb: the text
    as bytes)"""
    k0 = h & ~15
    lim = h + d + 16
    end = k0 + 16 * ((lim - k0) // 16) + 16                            # one past the last symbol the walk looks at (lim >= k0)
    stop = min(end, n - A)                                             # (B < A: suffix(B) is the longer)
    if stop > k0:
        a, b = Tb[A + k0: A + stop], Tb[B + k0: B + stop]
        if a != b:
            x = int.from_bytes(a, "big") ^ int.from_bytes(b, "big")    # the first symbol that differs: the highest set byte
            m = len(a) - 1 - (x.bit_length() - 1) // 8
            return a[m] < b[m]
    if n - A < end:
        return True                                                    # suffix(A) ends first: the shorter is the smaller
    return None


def _chain_round(T, Tb, n, sa, rk, h, mutant, tally):
    """the chain rule over every group of the round: per-suffix replacement of rank 2 (or -1), tallies candidates / taken"""
    r = rk[sa]
    head = np.ones(n, dtype=bool)
    head[1:] = r[1:] != r[:-1]
    starts = np.flatnonzero(head)
    sizes = np.diff(np.append(starts, n))
    gid = np.cumsum(head) - 1
    mn = np.minimum.reduceat(sa, starts).astype(np.int64)
    mx = np.maximum.reduceat(sa, starts).astype(np.int64)
    L = sizes.astype(np.int64)
    cand = L >= 2
    span = mx - mn
    Lm1 = np.maximum(L - 1, 1)
    cand &= span % Lm1 == 0
    d = span // Lm1
    cand &= (d >= 1) & (d <= CHAIN_DMAX)
    ncand = int(cand.sum())
    repl = np.full(n, -1, dtype=np.int64)
    if not ncand:
        return repl
    tally[1] += ncand
    member = cand[gid]
    v = sa[member].astype(np.int64)
    g = gid[member]
    dv, mnv, mxv = d[g], mn[g], mx[g]
    ok = np.ones(v.size, dtype=bool)
    if mutant != "lattice":
        ok &= (v - mnv) % dv == 0
    if mutant != "u":
        need = (v + 2 * dv < mxv) if mutant == "u_short" else (v + 2 * dv <= mxv)
        for dd in np.unique(dv[need]):
            dd = int(dd)
            c = np.concatenate(([0], np.cumsum(T[:-dd] != T[dd:])))
            sel = need & (dv == dd)
            vs = v[sel]
            ok[sel] &= (c[vs + dd] - c[vs]) == 0
    bad = np.zeros(len(starts), dtype=bool)
    bad[g[~ok]] = True
    good = np.flatnonzero(cand & ~bad)
    desc = {}
    for q in good:
        A, dq = int(mx[q]), int(d[q])
        less = _direction(Tb, n, A, A - dq, h, dq)
        if less is None:
            continue
        if mutant == "direction":
            less = not less
        desc[int(q)] = less
    if not desc:
        return repl
    tally[0] += len(desc)
    qs = np.fromiter(desc.keys(), dtype=np.int64, count=len(desc))
    isdesc = np.zeros(len(starts), dtype=bool)
    isdesc[qs] = np.fromiter(desc.values(), dtype=bool, count=len(desc))
    chain = np.zeros(len(starts), dtype=bool)
    chain[qs] = True
    pos = np.flatnonzero(chain[gid])
    vv = sa[pos].astype(np.int64)
    gg = gid[pos]
    at = (vv - mn[gg]) // d[gg]                                        # (integer division, as the kernel: off-lattice members with
    Lg = (mx[gg] - mn[gg]) // d[gg] + 1                                #  the lattice check dropped share a place)
    repl[vv] = np.where(isdesc[gg], Lg - 1 - at, at)
    return repl


def as_text(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data.astype(np.uint8)


def model_sa(data, chain_min=CHAIN_MIN, round_mask=CHAIN_ROUNDS, start="text", mutant=None):
    """the general sorter's suffix array of one block, with the chain rule as the kernels apply it (Result.sa None: the
    sorter would return its error, ties left that no depth parts).
    start: "text" (the default schedule), "isa" (sorter 2: doubling from depth 5), "resume" (doubling from SS_TOL_CAP)."""
    return model_schedules(data, [(chain_min, round_mask)], start, mutant)[0]


def model_schedules(data, schedules, start="text", mutant=None):
    """model_sa for several attempt schedules [(chain_min, round_mask), ...] of one block: the rounds up to the first one in
    which two schedules decide differently are run once"""
    T = as_text(data)
    n = len(T)
    if n == 0:
        return [Result(np.zeros(0, dtype=np.int64), 0, 0, 0, 0) for _ in schedules]
    R = prefix_ranks(T)
    Tb = T.tobytes()
    depth = SS_TOL_CAP if start == "resume" else 5
    rk = R.at(depth)
    # state: sa, rk, depth, isa mode, rounds, text rounds, doubling rounds, attempts, [taken, candidates]
    stack = [(list(range(len(schedules))), [np.argsort(rk), rk, depth, start in ("isa", "resume"), 0, 0, 0, 0, [0, 0]])]
    out = [None] * len(schedules)
    while stack:
        which, st = stack.pop()
        sa, rk, depth, mode_isa, rounds, text_rounds, isa_rounds, attempts, tally = st
        while True:
            rounds += 1
            r = rk[sa]
            head = np.ones(n, dtype=bool)
            head[1:] = r[1:] != r[:-1]
            tail = np.ones(n, dtype=bool)
            tail[:-1] = head[1:]
            live = n - int((head & tail).sum())
            if live == 0 or depth >= 2 * n + 16:                       # depth past the block: the sorter's error return (only a
                res = sa if live == 0 else None                        # wrong rule gets there: ties that no depth parts)
                for k in which:
                    out[k] = Result(res, tally[0], tally[1] - tally[0], rounds, attempts)
                break
            if not mode_isa and ((rounds == 1 and live > 0.25 * n) or text_rounds >= 3):
                mode_isa = True
            if not mode_isa:
                depth += 3
                text_rounds += 1
                rk = R.at(depth)
                sa = np.argsort(rk)
                continue
            decide = [bool(cm > 0 and live >= cm and isa_rounds < 32 and (rm >> isa_rounds) & 1 and
                           (isa_rounds == 0 or live >= 0.5 * n)) for cm, rm in (schedules[k] for k in which)]
            if any(decide) and not all(decide):                        # the schedules part here: the others go on later
                rest = [k for k, c in zip(which, decide) if not c]
                stack.append((rest, [sa, rk, depth, mode_isa, rounds - 1, text_rounds, isa_rounds, attempts, list(tally)]))
                which = [k for k, c in zip(which, decide) if c]
                decide = [True]
            # (a branch pushed above re-runs this round's rank-pass bookkeeping: rounds - 1)
            isa_rounds += 1
            r2 = _shift(rk, depth, n)
            if decide[0]:
                attempts += 1
                repl = _chain_round(T, Tb, n, sa, rk, depth, mutant, tally)
                r2 = np.where(repl >= 0, repl, r2)
            sa, rk = _dense(rk, r2, n)
            depth *= 2
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the corpus: random mosaics of what chain groups are made of, small blocks (shared with the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------------
def _word(rng, p):
    al = int(rng.choice([2, 3, 4, 256]))
    return rng.integers(0, al, p, dtype=np.uint8)


def _piece(rng, m, pieces):
    kind = int(rng.integers(0, 7))
    if kind <= 1:                                                      # a periodic stretch
        p = int(rng.integers(1, 41))
        return np.resize(_word(rng, p), m)
    if kind == 2:                                                      # a run
        return np.full(m, int(rng.integers(0, 256)), dtype=np.uint8)
    if kind == 3 and pieces:                                           # a copy of an earlier piece
        return np.resize(pieces[int(rng.integers(0, len(pieces)))], m)
    if kind == 4:                                                      # a periodic stretch with one byte changed (often near its end)
        p = int(rng.integers(1, 41))
        seg = np.resize(_word(rng, p), m).copy()
        at = int(rng.choice([rng.integers(0, m), m - 1 - rng.integers(0, min(m, 2 * p + 1))]))
        seg[at] ^= np.uint8(int(rng.integers(1, 256)))
        return seg
    if kind == 5:                                                      # a phrase at a fixed stride, other bytes between
        ph = _word(rng, int(rng.integers(4, 40)))
        stride = len(ph) + int(rng.integers(1, 60))
        seg = rng.integers(0, int(rng.choice([2, 4, 256])), m, dtype=np.uint8)
        for o in range(0, m - len(ph) + 1, stride):
            seg[o:o + len(ph)] = ph
        return seg
    return rng.integers(0, int(rng.choice([2, 4, 256])), m, dtype=np.uint8)   # random bytes


def mosaic(seed, n=None):
    """one corpus block: pieces glued up to n bytes (n <= 4096 drawn from the seed when not given); a quarter of the blocks
    start with a periodic stretch, a quarter end with one (the direction walk runs off the block)"""
    rng = np.random.default_rng(seed)
    if n is None:
        n = int(rng.choice([rng.integers(24, 300), rng.integers(300, 1200), rng.integers(1200, 4097)], p=[0.45, 0.4, 0.15]))
    x = np.empty(n, dtype=np.uint8)
    pieces = []
    o = 0
    first = rng.random() < 0.25
    last = rng.random() < 0.25
    while o < n:
        m = int(min(n - o, rng.integers(8, max(9, n // 2))))
        if (first and o == 0) or (last and o + m >= n):
            seg = np.resize(_word(rng, int(rng.integers(1, 41))), m)
        else:
            seg = _piece(rng, m, pieces)
        x[o:o + m] = seg
        pieces.append(seg[:64])
        o += m
    return x


# corpus seeds whose block gives a wrong suffix array (or ties no depth parts) under a mutant of the rule with a chain attempt in
# every doubling round, from a search over seeds 0 .. 19 999 (mutant: [(seed, block length)]).  Dropping the lattice check is
# wrong on 12 of those 20 000 blocks: an off-lattice member shares a place in the chain with a lattice one, or takes a place
# whose suffix it is not.  The other three mutants are wrong on hundreds to thousands of them.
ADVERSARIAL = {
    "lattice": [(9465, 41), (11332, 114), (6587, 120), (9580, 206), (3122, 380)],
    "u": [(46, 162), (24, 597), (61, 636)],
    "u_short": [(46, 162), (70, 202), (83, 584)],
    "direction": [(6, 146), (1, 154), (8, 222)],
}


def adversarial_blocks():
    """the distinct blocks of ADVERSARIAL, [(seed, block)]"""
    seen = {}
    for lst in ADVERSARIAL.values():
        for seed, n in lst:
            seen[seed] = mosaic(seed)
    return sorted(seen.items())
