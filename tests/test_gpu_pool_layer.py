"""GPU (fp32): packed scheduler steps through the fla layer and the GPT host on a `PagedDecodeCache` -- every request's rows against
`orc.fla_layer_forward` over that request's own sequence (the bound `test_fla_layer_exact_decoding` holds the cached layer to), against
the same request alone on a one-slot cache, and `GPT_MHLA.serve` teacher-forced against one plain forward per request."""
import functools

import pytest
import torch

from decode_util import layer_inputs
from gpu_util import DEV, check, launches, poison, _fla_layer
from oracle import mhla_oracle as orc

pytestmark = pytest.mark.gpu

OPTS = [{}, {"num_kv_heads": 1, "grouped_state": True}, {"use_output_gate": False}]
IDS = ["default", "grouped-state", "no-output-gate"]
# three scheduler steps: (slots, cu).  Slot 3: 70 + 59 + 1 tokens; slot 0: 5 + 1; slot 1, a fresh 130-token prompt in step two, + 1
STEPS = [((3, 0), (0, 70, 75)), ((0, 3, 1), (0, 1, 60, 190)), ((1, 3), (0, 1, 2))]
TOTAL = {3: 130, 0: 6, 1: 131}
POISON = 0x7FC0BEEF   # a NaN with a payload nothing computes


def slices(slot):
    """(step, first row in the step's pack, first token of the request, tokens) of every step the request in `slot` takes part in."""
    out, at = [], 0
    for i, (slots, cu) in enumerate(STEPS):
        if slot in slots:
            b = slots.index(slot)
            out.append((i, cu[b], at, cu[b + 1] - cu[b]))
            at += cu[b + 1] - cu[b]
    return out


@functools.lru_cache(maxsize=None)
def batched(case):
    """The three steps on one cache of four slots, run once per layer configuration and shared: (the layer, every request's input,
    every step's output rows, what the test of the steps asserts about launches, lengths, pages and poison)."""
    from mhla_amd import modules
    poison()
    m = _fla_layer(**OPTS[case])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).eval()
    x = {slot: layer_inputs(1, n, 50 + slot).to(DEV) for slot, n in TOTAL.items()}
    cache = modules.PagedDecodeCache(n_slots=4, capacity_chunks=32, n_pages=12)
    outs, ran, kept = [], [], None
    with torch.no_grad():
        for i, (slots, cu) in enumerate(STEPS):
            pack = torch.cat([x[s][:, t0:t0 + n] for s in slots for j, _, t0, n in slices(s) if j == i], dim=1)
            cache.schedule(slots, cu)
            got = []
            ran.append(launches(lambda: got.append(m(pack, past_key_values=cache, use_cache=True)[0])))
            outs.append(got[0])
            if i == 0:
                # slot 2 and every page no step has assigned yet start as poison: pages a later step assigns are written before they
                # are read, and what no step assigns keeps these bits
                pool = cache.pool(0)
                free = sorted(pool.free)
                assert free == list(range(3, 12)) and cache.lengths == (5, 0, 0, 70)
                for t in (pool.pages[3:], pool.P[2], pool.Cur[2]):
                    t.view(torch.int32).fill_(POISON)
                kept = lambda: [pool.pages[7:].view(torch.int32), pool.P[2].view(torch.int32), pool.Cur[2].view(torch.int32)]
    return m, sd, x, outs, ran, cache, kept


def rows_of(outs, slot):
    return torch.cat([outs[i][:, r0:r0 + n] for i, r0, _, n in slices(slot)], dim=1)


@pytest.mark.parametrize("case", range(3), ids=IDS)
def test_three_steps_against_the_oracle(case):
    m, sd, x, outs, ran, cache, kept = batched(case)
    opts = {k: v for k, v in OPTS[case].items() if k != "grouped_state"}
    for slot in TOTAL:
        want = orc.fla_layer_forward(sd, x[slot].cpu(), 2, 64, 128, norm_eps=1e-6, **opts)
        check(f"o (the request of slot {slot}, step by step)", rows_of(outs, slot), want, 1e-4)
    assert cache.lengths == (6, 131, 0, 130) and cache.get_seq_length() == 131 and len(cache) == 1
    pool = cache.pool(0)
    assert pool.dims == (4, 1 if case == 1 else 2, 32, 64, 128) and cache.pages_free == 12 - 7
    for r in ran:
        assert r.get("k_fr_decode") == 1 and "k_fmap_rotary" not in r, r
    assert all(bool((t == POISON).all()) for t in kept()), "slot 2 and the pages no step assigned keep their poison bits"
    assert sorted(p for row in pool.table for p in row if p >= 0) == list(range(7))


@pytest.mark.parametrize("case", range(3), ids=IDS)
def test_every_request_as_if_alone(case):
    """The same slices with one request alone on a one-slot cache: what its neighbours in the pack and the pool do changes nothing."""
    from mhla_amd import modules
    m, sd, x, outs, ran, cache, kept = batched(case)
    poison()
    with torch.no_grad():
        for slot in TOTAL:
            own = modules.PagedDecodeCache(n_slots=1, capacity_chunks=32, n_pages=3)
            alone = []
            for _, _, t0, n in slices(slot):
                own.schedule([0], [0, n])
                alone.append(m(x[slot][:, t0:t0 + n], past_key_values=own, use_cache=True)[0])
            assert own.lengths == (TOTAL[slot],)
            check(f"slot {slot}: batched against alone", rows_of(outs, slot), torch.cat(alone, dim=1).cpu(), 1e-4)


def test_the_host_serves_requests():
    from mhla_amd.hosts.gpt import GPT_MHLA
    from mhla_amd.modules import PagedDecodeCache
    poison()
    torch.manual_seed(5)
    model = GPT_MHLA(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, max_seq_len=2048, exact_decoding=True).to(DEV).eval()
    g = torch.Generator().manual_seed(6)
    prompts = [torch.randint(0, 512, (n,), generator=g) for n in (70, 5, 130, 64, 1)]
    cache = PagedDecodeCache(n_slots=2, capacity_chunks=32, n_pages=6)
    ids, logits = model.serve(prompts, 6, n_slots=2, n_pages=6, step_tokens=48, return_logits=True, cache=cache)
    assert len(ids) == len(logits) == 5
    with torch.no_grad():
        for r, (p, new, lg) in enumerate(zip(prompts, ids, logits)):
            assert tuple(new.shape) == (6,) and new.dtype == torch.long and tuple(lg.shape) == (6, 512)
            assert torch.equal(new, lg.argmax(-1)), f"request {r}: every id is the argmax of the logits returned for it"
            # teacher-forced: one plain forward over prompt + emitted ids; row P - 1 + j is what id j was picked from
            full = model(torch.cat([p.to(DEV), new])[None])[0]
            check(f"logits of request {r}: served against one forward", lg, full[len(p) - 1:len(p) + 5].cpu(), 1e-4)
    assert len(cache) == 2 and cache.pool(0).table == cache.pool(1).table, "identical page-rule calls, identical tables"
    assert cache.pool(0).lengths == cache.pool(1).lengths == (0, 0)
    assert cache.pages_free == cache.pool(1).pages_free == 6, "all pages are free after the last release"
