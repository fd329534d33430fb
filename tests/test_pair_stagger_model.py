"""A model of the pair kernels' staggered schedule (merson_pair),
restated from the table of LDS accesses beside the z-loop; no GPU.

Every wave runs, per plane step mm: T (stage A's input of plane mm + 1 into lA), A (stage A at
plane mm, writes lB), B (stage B at plane mm - 1).  The early half (waves 0-3) passes the step's
barrier after B, the late half (waves 4-7) between A and B; the chunk's last step (mm == ke) has no
barrier in either half.  GLB kernels (the GLX route) keep stage B's gl in lA, field 2: the x/y
neighbour reads of that plane are hoisted ahead of the late half's barrier, in both halves.

For each half the model lists, in program order, the barriers and the LDS accesses (ring, slot,
field, own position or a neighbour's, the plane expected or written).  The k-th barrier of every
wave is the same event, so an access lies in the barrier interval numbered by the barriers its
half has passed.  Asserted for chunks of 1 .. 9 and 16 planes of a 16-plane slab, at walls and
between slabs, for the two-plane boundary chunks and an empty chunk:

  (i)   both halves pass equally many barriers;
  (ii)  no read of another thread's position shares an interval with a write to that ring slot and
        field, and it finds the plane it expects, written in an earlier interval;
  (iii) with the hoist taken out of the model, (ii) fails for GLB (and only for GLB)."""
import itertools

import pytest

N3 = 16
KZS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16]


def _chunks(kz, has_below, has_above):
    """(kb, ke) of a slab's chunks: the whole slab cut into kz planes"""
    return [(kb, min(kb + kz, N3)) for kb in range(0, N3, kz)]


def _schedule(kb, ke, has_below, has_above, glb, late, stagger=True, hoist=True):
    """one wave's events in program order: ("bar",) or (kind, ring, slot, field, who, plane) with
    kind "r" / "w" and who "own" / "nbr" -- merson_pair's prologue and z-loop for the chunk
    [kb, ke) of a slab of N3 planes"""
    ev = []
    if kb >= ke:
        return ev                                    # an empty chunk: no prologue, no loop
    wlo, whi = not has_below, not has_above
    mA0 = kb - 1 if kb > 0 else (0 if wlo else -1)
    mA1 = ke if ke < N3 else (N3 - 1 if whi else N3)
    mlast = min(mA1 + 1, N3 - 1 if whi else N3 + 1)
    nbq = 2 if glb else 3
    slot = lambda p: (p - mA0) % 3
    late = late and stagger
    # prologue: planes mA0 - 1 (or plane 0's mirror at the bottom wall) and mA0 into slots 2 and 0
    for q in range(3):
        ev.append(("w", "lA", 2, q, "own", mA0 - 1))
        ev.append(("w", "lA", 0, q, "own", mA0))
    ev.append(("bar",))
    for mm in range(mA0, ke + 1):
        kB = mm - 1
        # T: the top
        if glb:
            ev.append(("r", "lA", slot(mm + 1), 2, "own", mm - 2))        # glm (pair 4+5; a register in 2+3)
        if mm + 1 <= mlast:
            for q in range(3):
                ev.append(("w", "lA", slot(mm + 1), q, "own", mm + 1))    # the extras' too (last wave)
        # A: stage A at plane mm
        if mm <= mA1:
            if mm == N3 - 1 and whi:
                for q in range(3):
                    ev.append(("w", "lA", slot(mm + 1), q, "own", mm + 1))   # top wall: the ghost plane
            for q in range(3):
                ev.append(("r", "lA", slot(mm), q, "nbr", mm))            # x/y neighbours, mirrors
                for d in (-1, 0, 1):
                    ev.append(("r", "lA", slot(mm + d), q, "own", mm + d))
            for q in range(nbq):
                ev.append(("w", "lB", slot(mm), q, "own", mm))
                if mm == 0 and wlo:
                    ev.append(("w", "lB", slot(mm - 1), q, "own", mm - 1))   # bottom wall: the mirror plane
        runs_b = kB >= kb
        if stagger and hoist and glb and runs_b:
            ev.append(("r", "lA", slot(kB), 2, "nbr", kB))                # the hoisted gl neighbours
        if late and mm != ke:
            ev.append(("bar",))
        # B: stage B at plane kB
        if runs_b:
            if kB == N3 - 1 and whi:
                for q in range(nbq):
                    ev.append(("w", "lB", slot(kB + 1), q, "own", kB + 1))   # top wall: the ghost plane
            for q in range(nbq):
                ev.append(("r", "lB", slot(kB), q, "nbr", kB))
                for d in (-1, 0, 1):
                    ev.append(("r", "lB", slot(kB + d), q, "own", kB + d))
            if glb:
                if not (stagger and hoist):
                    ev.append(("r", "lA", slot(kB), 2, "nbr", kB))
                ev.append(("r", "lA", slot(kB), 2, "own", kB))
                ev.append(("r", "lA", slot(kB + 1), 2, "own", kB + 1))
        if mm == ke:
            break
        if not late:
            ev.append(("bar",))
    return ev


def _check(kb, ke, has_below, has_above, glb, stagger=True, hoist=True):
    """(barriers of the early half, of the late half, hazards) of one chunk"""
    halves = [_schedule(kb, ke, has_below, has_above, glb, late, stagger, hoist) for late in (False, True)]
    nbar = [sum(1 for e in h if e[0] == "bar") for h in halves]
    writes, reads = {}, []          # (ring, slot, field) -> [(interval, plane)]; neighbour reads
    for h in halves:
        iv = 0
        for e in h:
            if e[0] == "bar":
                iv += 1
            elif e[0] == "w":
                writes.setdefault(e[1:4], []).append((iv, e[5]))
            elif e[4] == "nbr":
                reads.append((e[1:4], iv, e[5]))
    hazards = []
    for key, iv, plane in reads:
        ws = writes.get(key, [])
        if any(w == iv for w, _ in ws):
            hazards.append((key, iv, plane, "a write in the read's interval"))
            continue
        before = [(w, p) for w, p in ws if w < iv]
        if not before or {p for w, p in before if w == max(b[0] for b in before)} != {plane}:
            hazards.append((key, iv, plane, "not the expected plane"))
    return nbar[0], nbar[1], hazards


def _cases():
    for kz, below, above in itertools.product(KZS, (False, True), (False, True)):
        for kb, ke in _chunks(kz, below, above):
            yield kb, ke, below, above
    for below, above in ((True, False), (False, True), (True, True)):
        # the two-plane boundary chunks (kb = chunk (n3 - 2), ke = kb + 2) and the interior between
        yield 0, 2, below, above
        yield N3 - 2, N3, below, above
        yield 2, N3 - 2, below, above
    yield 5, 5, True, True                           # an empty chunk


CASES = sorted(set(_cases()))


def test_cases_cover_the_paths():
    lengths = {ke - kb for kb, ke, _, _ in CASES}
    assert lengths >= set(KZS) | {0, 12}
    assert any(kb == 0 and not b for kb, ke, b, a in CASES) and any(ke == N3 and not a for kb, ke, b, a in CASES)
    assert any(kb == 0 and b for kb, ke, b, a in CASES) and any(ke == N3 and a for kb, ke, b, a in CASES)


@pytest.mark.parametrize("glb", [True, False], ids=["glb", "noglb"])
def test_halves_pass_equally_many_barriers(glb):
    for kb, ke, below, above in CASES:
        early, late, _ = _check(kb, ke, below, above, glb)
        assert early == late, (kb, ke, below, above)
        # the prologue's and one per step but the last; none for an empty chunk
        mA0 = kb - 1 if kb > 0 else (-1 if below else 0)
        assert early == (ke - mA0 + 1 if kb < ke else 0), (kb, ke, below, above)
        # the unstaggered schedule passes the same number
        assert _check(kb, ke, below, above, glb, stagger=False)[:2] == (early, early)


@pytest.mark.parametrize("glb", [True, False], ids=["glb", "noglb"])
def test_no_neighbour_read_meets_a_write(glb):
    for kb, ke, below, above in CASES:
        assert _check(kb, ke, below, above, glb)[2] == [], (kb, ke, below, above)
        assert _check(kb, ke, below, above, glb, stagger=False)[2] == [], (kb, ke, below, above)


def test_without_the_hoist_the_model_sees_the_gl_hazard():
    hit = {}
    for kb, ke, below, above in CASES:
        hz = _check(kb, ke, below, above, True, hoist=False)[2]
        # only stage B's gl neighbours in lA (field 2), and only behind the late half's barrier
        assert all(key[0] == "lA" and key[2] == 2 for key, _, _, _ in hz)
        hit[(kb, ke, below, above)] = len(hz)
        # kernels that keep stage B's gl in lB have no hoist to lose
        assert _check(kb, ke, below, above, False, hoist=False)[2] == []
    # a late stage B of step mm (kb + 1 <= mm < ke: it runs, behind a barrier) meets the early
    # half's top of step mm + 1 where that top still stores (mm + 2 <= mlast): the chunks with
    # ke >= kb + 2 and kb + 3 <= mlast, and no others
    for (kb, ke, below, above), n in hit.items():
        mA1 = ke if ke < N3 else (N3 if above else N3 - 1)
        mlast = min(mA1 + 1, N3 + 1 if above else N3 - 1)
        assert (n > 0) == (ke - kb >= 2 and kb + 3 <= mlast), (kb, ke, below, above)
    assert sum(1 for n in hit.values() if n) > len(hit) // 2
    assert hit[(0, N3, False, False)] >= N3 - 3
