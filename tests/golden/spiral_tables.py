"""Synthetic spiral index tables for the SpiralConv kernel tests.

TEST INFRASTRUCTURE.  The craniofacial template is a tame input for the data
gradient: at most 7 rows on a (vertex, slot) key, no row naming a vertex
twice, no vertex outside every spiral, per-vertex fan-in of the Enblock tables
12 / 6 / 6 / 6.  Each generator here returns an ``[rows, 9]`` int64 table over
``vsrc`` source vertices that has one property the template lacks, and ASSERTS
that property before returning, so that a later edit cannot quietly turn it
into a tame table (``tests/test_spiral_tables_host.py`` runs every generator
on the CPU).  ``rows`` is unrelated to ``vsrc``: ``rows == vsrc`` is the decoder
form, ``rows ~ vsrc / 4`` the Enblock form, and ``rows == 3 * vsrc`` is allowed
by every entry point.

Terms: a *key* is a pair (u, s) of source vertex and spiral slot; its *list*
is the rows r with ``table[r, s] == u`` (``topology.inverse_spiral``).  The
kernels keep the first ``INV_HEAD`` = 4 rows of a list inline and walk the rest
in a lane-divergent loop.  The *fan-in* of u is the number of positions (r, s)
naming it (``topology.inverse_flat``'s list length).

Everything is a deterministic function of the arguments (numpy RandomState).
"""
import numpy as np

SEQ = 9
INV_HEAD = 4  # == CFSD_INV_HEAD (asserted against the header by the host test)
GAP_RUN_MIN = 512  # vertex count from which a gaps table has its run of 64 absent vertices


def key_counts(table, vsrc):
    """List length of every key: [vsrc, seq]."""
    table = np.asarray(table, np.int64)
    seq = table.shape[1]
    keys = (table * seq + np.arange(seq)[None, :]).reshape(-1)
    return np.bincount(keys, minlength=vsrc * seq).reshape(vsrc, seq)


def fan_in(table, vsrc):
    return np.bincount(np.asarray(table, np.int64).reshape(-1), minlength=vsrc)


def _check(table, rows, vsrc):
    assert table.shape == (rows, SEQ) and table.dtype == np.int64
    assert table.min() >= 0 and table.max() < vsrc
    return table


def gap_vertices(vsrc):
    """The vertices the ``gaps`` tables keep out of every spiral: 0, vsrc - 1 and
    (from ``GAP_RUN_MIN`` vertices on) 64 consecutive ones starting at a multiple
    of 32 in the second quarter."""
    absent = [0, vsrc - 1]
    if vsrc >= GAP_RUN_MIN:
        start = (vsrc // 4) // 32 * 32
        absent += list(range(start, start + 64))
    return np.array(sorted(set(absent)), np.int64)


def _spread(rs, rows, eligible):
    """A table whose every column walks a random permutation of ``eligible``:
    every key of an eligible vertex gets floor or ceil(rows / len(eligible)) rows."""
    cols = []
    for _ in range(SEQ):
        perm = rs.permutation(eligible)
        cols.append(perm[np.arange(rows) % len(perm)])
    return np.stack(cols, 1).astype(np.int64)


def random(rows, vsrc, seed=0):
    """Independent uniform draws with replacement: repeated vertices inside a
    row, Poisson fan-in."""
    rs = np.random.RandomState(seed)
    t = rs.randint(0, vsrc, size=(rows, SEQ)).astype(np.int64)
    if not any(len(set(r)) < SEQ for r in t):  # (certain unless vsrc is huge and rows tiny)
        t[0, 1] = t[0, 0]
    assert any(len(set(r)) < SEQ for r in t), "no row repeats a vertex"
    return _check(t, rows, vsrc)


def hubs(rows, vsrc, seed=0):
    """A handful of hub vertices receive about half of all entries, each on
    three slots (hub k on the slots s with s % 3 == k % 3), so a hub key's list
    is far longer than the inline head; the neighbouring keys (u, s +- 1) and
    (u - 1, s) are empty and (u + 1, s) has exactly one row.  Inside the hub's
    aligned group of 16 vertices the list lengths of one slot therefore include
    0, 1 and more than 4: divergent trip counts of the tail walk inside one
    MFMA row tile.  Needs vsrc >= 160 and rows >= 160."""
    assert vsrc >= 160 and rows >= 160
    rs = np.random.RandomState(seed)
    n_hubs = 5
    hub = np.array([((k + 1) * vsrc // (n_hubs + 1)) // 16 * 16 + 5 for k in range(n_hubs)], np.int64)
    assert len(set(hub)) == n_hubs and hub.max() + 1 < vsrc
    near = np.concatenate([hub - 1, hub, hub + 1])
    eligible = np.setdiff1d(np.arange(vsrc), near)
    t = _spread(rs, rows, eligible)
    for s in range(SEQ):
        mine = hub[np.arange(n_hubs) % 3 == s % 3]
        order = rs.permutation(rows)
        half = order[:rows // 2]
        t[half, s] = mine[np.arange(len(half)) % len(mine)]
        t[order[rows // 2:rows // 2 + len(mine)], s] = mine + 1  # exactly one row on (u + 1, s)
    cnt = key_counts(t, vsrc)
    assert cnt.max() > 8 * INV_HEAD, "no long list"
    share = fan_in(t, vsrc)[hub].sum() / t.size
    assert 0.4 <= share <= 0.6, share
    for k, u in enumerate(hub):
        for s in range(SEQ):
            if s % 3 != k % 3:
                assert cnt[u, s] == 0
                continue
            assert cnt[u, s] > INV_HEAD and cnt[u + 1, s] == 1 and cnt[u - 1, s] == 0
            for ds in (-1, 1):
                if 0 <= s + ds < SEQ:
                    assert cnt[u, s + ds] <= 1
            group = cnt[u // 16 * 16:u // 16 * 16 + 16, s]
            assert (group == 0).any() and (group == 1).any() and (group > INV_HEAD).any()
    return _check(t, rows, vsrc)


def head_edge_keys(vsrc):
    """The keys ``head_edge`` sizes, as (u, s, list length): lengths 3, 4, 5, 6
    on four consecutive vertices of one aligned group of 16: in the first tile
    of dx rows, in the middle, and among the last five vertices (the last,
    partial tile of an odd vertex count); never vertex 0 or vsrc - 1."""
    assert vsrc >= 37
    out = []
    for place, u0 in enumerate((1, vsrc // 2 // 16 * 16 + 6, vsrc - 5)):
        for j, n in enumerate((3, 4, 5, 6)):
            out.append((u0 + j, (2 * place + 3 * j) % SEQ, n))
    return out


def head_edge(rows, vsrc, seed=0, gaps=True):
    """Chosen keys with exactly 3, 4, 5 and 6 rows -- both sides of the inline
    head of 4 -- in the first vertex tile, the last one and the middle
    (``head_edge_keys``), on neighbouring vertices, so adjacent lanes walk 0, 0,
    1 and 2 tail entries.  With ``gaps`` the vertices of ``gap_vertices`` are in
    no spiral: the first and the last dx row, and 64 consecutive ones from a
    multiple of 32 on (whole dx row tiles of every tiling are all-absent)."""
    assert rows >= 37
    rs = np.random.RandomState(seed)
    chosen = head_edge_keys(vsrc)
    special = np.array(sorted({u for u, _, _ in chosen}), np.int64)
    absent = gap_vertices(vsrc) if gaps else np.zeros(0, np.int64)
    assert not set(special) & set(absent)
    eligible = np.setdiff1d(np.arange(vsrc), np.concatenate([special, absent]))
    t = _spread(rs, rows, eligible)
    for s in range(SEQ):
        mine = [(u, n) for u, ss, n in chosen if ss == s]
        order = rs.permutation(rows)
        at = 0
        for u, n in mine:
            t[order[at:at + n], s] = u
            at += n
        assert at <= rows
    cnt = key_counts(t, vsrc)
    for u, s, n in chosen:
        assert cnt[u, s] == n, (u, s, n, cnt[u, s])
    for place in range(3):  # every length in every place
        assert sorted(n for _, _, n in chosen[4 * place:4 * place + 4]) == [3, 4, 5, 6]
    assert max(u for u, _, _ in chosen[:4]) < 16
    assert min(u for u, _, _ in chosen[8:]) >= vsrc - 5
    if gaps:
        assert_gaps(t, vsrc)
    return _check(t, rows, vsrc)


def assert_gaps(table, vsrc):
    f = fan_in(table, vsrc)
    assert f[0] == 0 and f[vsrc - 1] == 0
    if vsrc >= GAP_RUN_MIN:
        zero = np.concatenate([[0], (f == 0).astype(np.int64), [0]])
        edges = np.flatnonzero(np.diff(zero))
        runs = [(a, b - a) for a, b in zip(edges[::2], edges[1::2])]
        # (a run may begin earlier when its neighbours happen to be absent as well)
        assert any(-(-a // 32) * 32 + 64 <= a + n for a, n in runs), "no 64 absent vertices from a multiple of 32 on"


def one_vertex_rows(rows, vsrc, seed=0, every=7):
    """The ``random`` table with every ``every``-th row naming ONE vertex in
    all nine slots (the forward gathers one row nine times; the vertex gets a
    row on each of its nine keys)."""
    rs = np.random.RandomState(seed + 1)
    t = random(rows, vsrc, seed)
    same = np.arange(0, rows, every)
    t[same] = rs.randint(0, vsrc, size=len(same))[:, None]
    assert len(same) > 0 and all(len(set(t[r])) == 1 for r in same)
    return _check(t, rows, vsrc)


def fan_table(rows, vsrc, fan, seed=0):
    """A table whose largest per-vertex fan-in is EXACTLY ``fan`` (the width
    class of ``topology.inverse_flat``: widths 4, 8, 12, 16, and none from 17
    on by default; the full-table entry points take width 20 through
    ``inverse_flat(..., max_width=20)``, and fan 17 .. 20 builds as well:
    ``tests/test_exact_values_host.py``).  Four neighbouring vertices in the middle get fan, fan - 1, fan - 2
    and fan - 3 positions (every padding of the last int4 group of a flat-list
    row), the vertices of ``gap_vertices`` none, a tenth of the rest a uniform
    draw from 0 .. fan (as far as the positions last) and the others an even
    share.  Positions are shuffled, so rows repeat vertices."""
    rs = np.random.RandomState(seed)
    total = rows * SEQ
    absent = gap_vertices(vsrc)
    u0 = vsrc // 2 // 16 * 16 + 6
    top = np.arange(u0, u0 + 4)
    assert not set(top) & set(absent)
    want = np.zeros(vsrc, np.int64)
    want[top] = [fan, fan - 1, fan - 2, max(fan - 3, 1)]
    rest = rs.permutation(np.setdiff1d(np.arange(vsrc), np.concatenate([top, absent])))
    left = total - int(want.sum())
    assert left >= 0
    drawn = rs.randint(0, fan + 1, size=len(rest) // 10)
    drawn = drawn[np.cumsum(drawn) <= left // 2]
    want[rest[:len(drawn)]] = drawn
    rest, left = rest[len(drawn):], left - int(drawn.sum())
    base, extra = divmod(left, len(rest))
    assert base + (extra > 0) <= fan, "too many rows for this fan-in"
    want[rest] = base
    want[rest[:extra]] += 1
    flat = rs.permutation(np.repeat(np.arange(vsrc), want))
    t = flat.reshape(rows, SEQ).astype(np.int64)
    f = fan_in(t, vsrc)
    assert f.max() == fan and (f[top] == want[top]).all()
    assert_gaps(t, vsrc)
    return _check(t, rows, vsrc)
