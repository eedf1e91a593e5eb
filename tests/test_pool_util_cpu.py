"""The checkers of tests/pool_util.py, checked without a GPU and without the library (as tests/test_check_chunks_cpu.py does for
check_chunks): on a small pool of every kind built by `fill_pool` from a random compact state on the CPU, `check_pool` passes on the
untouched pool against its own `compact()` -- NaN poison included, bits compare equal --, raises on every single-bit flip (xor 1 on the
integer view) or edit of the host mirror of what a call must leave alone, naming the part and the slot or page, and lets a writable
page change."""
import pytest
import torch

from mhla_amd import CausalState, _lib
from pool_util import CAP, LENGTHS, N_PAGES, N_SLOTS, TABLE, VIEW, bits, check_pool, check_untouched, fill_pool, snapshot

KINDS = ["dense", "paged", "h16"]
PAGED = KINDS[1:]
STEP = (64, 6, 131)    # reach of a step on VIEW: the open chunks' pages 6, 4, 2 are writable, slot 4's finished 7, 5 are not
GROW = (64, 70, 131)   # slot 0 reaches chunk 1, which TABLE gives no page


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", load)


def make(kind):
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(s, generator=g)
    src = CausalState(r(3, 2, CAP, 8, 16), r(3, 2, 8, 16), r(3, 2, 8, 16), 0, 64, lengths=LENGTHS)
    pool = fill_pool(kind, src, VIEW, n_slots=N_SLOTS, table=TABLE, n_pages=N_PAGES)
    return pool, snapshot(pool), pool.at(VIEW).compact()


def flip(t):
    """xor 1 on the integer view of the first element of the view `t` of a pool's tensor"""
    bits(t).reshape(-1)[:1] ^= 1


def set_length(pool, slot, n):
    pool.lengths = tuple(n if s == slot else m for s, m in enumerate(pool.lengths))


def set_entry(pool, slot, j, page, host=True, dev=True):
    if host:
        pool.table[slot][j] = page
    if dev:
        pool.table_dev[slot, j] = page


def run(kind, change, how):
    """`check_pool` of VIEW at LENGTHS against the pool's own compact(), with the arguments `how`; `how["only"]`: `check_untouched` alone,
    with VIEW as the touched slots."""
    pool, before, ref = make(kind)
    change(pool)
    if how.get("only"):
        return check_untouched("call", pool, before, VIEW, **{a: b for a, b in how.items() if a != "only"})
    return check_pool("call", pool, before, ref, VIEW, LENGTHS, **how)


@pytest.mark.parametrize("kind", KINDS)
def test_an_untouched_pool_passes_poison_included(kind):
    pool, before, ref = make(kind)
    assert bool(torch.isnan(pool.P[1]).all()) and pool.pos.tolist()[1] == 0x7FC00000 and ref.lengths == LENGTHS
    check_pool("call", pool, before, ref, VIEW, LENGTHS)
    check_pool("call", pool, before, ref, VIEW, LENGTHS, touched=[3, 4], flagged=[1], reach=STEP)
    check_untouched("call", pool, before, ())


# (id, kinds, the change, what the message names, arguments of the check)
CAUGHT = [
    ("P-unnamed", KINDS, lambda p: flip(p.P[1]), "P of slot 1", {}),
    ("Cur-named-not-touched", KINDS, lambda p: flip(p.Cur[0]), "Cur of slot 0", dict(touched=[3, 4])),
    ("pos-unnamed", KINDS, lambda p: flip(p.pos[2]), "pos of slot 2", {}),
    ("full-unnamed", KINDS, lambda p: flip(p.full[1]), "full of slot 1", dict(flagged=[2])),
    ("lengths-unnamed", KINDS, lambda p: set_length(p, 1, 7), "lengths entry of slot 1", {}),
    ("S-unnamed", ["dense"], lambda p: flip(p.S[2, 1, 3]), "S of slot 2", {}),
    ("free-page", PAGED, lambda p: flip(p.pages[8]), "payload of page 8", dict(reach=STEP)),
    ("page-of-another-slot", PAGED, lambda p: flip(p.pages[7]), "payload of page 7", dict(touched=[3, 0], reach=STEP)),
    ("finished-page-of-a-touched-slot", PAGED, lambda p: flip(p.pages[5]), "payload of page 5", dict(only=True, reach=STEP)),
    ("page-outside-the-given-set", PAGED, lambda p: flip(p.pages[6]), "payload of page 6", dict(only=True, pages=[8])),
    ("table-row-unnamed", PAGED, lambda p: set_entry(p, 1, 0, 3), "table row of slot 1", {}),
    ("table_dev", PAGED, lambda p: set_entry(p, 3, 1, 9, host=False), "table_dev", {}),
    ("no-page-in-reach", PAGED, lambda p: None, "chunk 1 of slot 0, which the call reaches, has no page", dict(reach=GROW)),
    ("multiplier", ["h16"], lambda p: flip(p.page_mult[7, 1]), "multipliers of page 7", dict(only=True, reach=STEP)),
    ("multiplier-free-page", ["h16"], lambda p: flip(p.page_mult[8, 1]), "multipliers of page 8", dict(reach=STEP)),
    ("P-touched", KINDS, lambda p: flip(p.P[3]), "P of slot 3", {}),
    ("chunk-touched", ["dense"], lambda p: flip(p.S[4, 0, 1]), "S of slot 4", {}),
    ("chunk-touched", PAGED, lambda p: flip(p.pages[5]), r"chunk 1 of slot 4 \(page 5\)", {}),
    ("pos-touched", KINDS, lambda p: p.pos[0].add_(1), "pos of slot 0 is 6, the compact state's 5, expected 5", {}),
]


@pytest.mark.parametrize("kind, change, names, how", [pytest.param(k, *c[2:], id=f"{c[0]}-{k}") for c in CAUGHT for k in c[1]])
def test_every_change_a_call_must_not_make_is_caught(kind, change, names, how):
    with pytest.raises(AssertionError, match="call: .*" + names):
        run(kind, change, how)


@pytest.mark.parametrize("kind", KINDS)
def test_a_flag_of_a_flagged_slot_may_be_set(kind):
    run(kind, lambda p: flip(p.full[1]), dict(flagged=[1]))


def grow(pool):
    """slot 0 gets page 9 for chunk 1, and that page and the three open chunks' change"""
    set_entry(pool, 0, 1, 9)
    for p in (6, 4, 2, 9):
        flip(pool.pages[p])
        if pool.page_mult is not None:
            flip(pool.page_mult[p])


@pytest.mark.parametrize("kind", PAGED)
def test_a_writable_page_may_change(kind):
    run(kind, lambda p: [flip(p.pages[q]) for q in (6, 4, 2)], dict(only=True, reach=STEP))
    run(kind, grow, dict(only=True, reach=GROW))
    run(kind, lambda p: flip(p.pages[8]), dict(only=True, pages=[8]))
    with pytest.raises(AssertionError, match="payload of page 9"):   # (the same growth, held to the reach of a step)
        run(kind, grow, dict(only=True, reach=STEP))
