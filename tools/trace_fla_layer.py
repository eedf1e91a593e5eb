"""Call trace of the fla layer `MHLA` and the `GPT_MHLA` host, to `diff` between two trees after a host-side refactor
(`profiles/fla_forward_refactor.md`).

Every operator name bound in `mhla_amd.modules.fla` is replaced by a spy that logs its arguments (per tensor: shape, stride, dtype
and a sha256 of its bytes; decode states and packed-sequence plans field by field; `repr` of everything else) and a hash of its
result, and calls through.  After every layer call the output, `mixing_matrix.data`, the cache's token counts and every field of
every decode state are hashed; the training cases add the input gradient and every parameter gradient.  Fixed seeds, one process,
one GPU.  Run both trees in ONE session: there two runs give one log, while between machines the `use_short_conv` cases vary with
the kernel `torch.nn.functional.conv1d` picks (`--no-conv-grads` leaves the `*_conv1d.weight` gradient lines out).

    python tools/trace_fla_layer.py --out trace.log [--no-conv-grads]
"""
import argparse
import hashlib
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mhla_amd.hosts import gpt as host  # noqa: E402
from mhla_amd.modules import fla  # noqa: E402
from mhla_amd.ops import CausalState, CausalVarlenPlan  # noqa: E402

DEV = "cuda"
SPIED = ("mhla_causal", "mhla_causal_normgate", "mhla_causal_state", "mhla_causal_prefill", "mhla_causal_step", "mhla_causal_extend",
         "mhla_causal_step_dev", "featmap_rotary", "rmsnorm_gate", "naive_recurrent_mhla", "causal_varlen_plan", "_mix2d")
LOG = []
SKIP_CONV_GRADS = False


def sha(t):
    b = t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()
    return hashlib.sha256(b).hexdigest()[:20]


def describe(x):
    if isinstance(x, torch.Tensor):
        return f"T{tuple(x.shape)}{tuple(x.stride())}{str(x.dtype)[6:]}#{sha(x)}"
    if isinstance(x, CausalState):
        return ("State(" + " ".join(f"{n}={describe(getattr(x, n))}" for n in ("S", "P", "Cur", "pos", "lengths", "seen", "stale")) + ")")
    if isinstance(x, CausalVarlenPlan):
        return f"Plan(cu={x.cu} chunk={x.chunk_size} table={describe(x.table)} loc={describe(x.loc)} seq={describe(x.seq)})"
    if isinstance(x, (tuple, list)):
        return "[" + ", ".join(describe(e) for e in x) + "]"
    return repr(x)


def log(line):
    LOG.append(line)


def spy(name, fn):
    def wrapped(*a, **kw):
        args = [describe(x) for x in a] + [f"{k}={describe(v)}" for k, v in kw.items()]
        log(f"  op {name}({'; '.join(args)})")
        res = fn(*a, **kw)
        log(f"  -> {describe(res)}")
        return res
    return wrapped


def log_cache(cache):
    if cache is None or not hasattr(cache, "states"):
        return
    log(f"  cache len={len(cache)} seen={cache._seen}")
    for i, entry in enumerate(cache.states):
        log(f"  cache[{i}] " + " ".join(f"{k}={describe(v)}" for k, v in entry.items()))


def warned(fn):
    """fn(), with every warning it raises logged: category, text and the frame it is attributed to."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            res = fn()
        except (ValueError, NotImplementedError, IndexError, TypeError, AssertionError) as e:   # a refusal is part of the trace
            res = None
            log(f"  raised {type(e).__name__}: {e}")
    for w in caught:
        if not issubclass(w.category, ResourceWarning):   # (the library loader's unclosed files: they name this checkout's path)
            log(f"  warning {w.category.__name__} at {os.path.basename(w.filename)}:{w.lineno}: {w.message}")
    return res


def layer_call(tag, m, x, cache=None, **kw):
    log(f"call {tag} x={describe(x)} " + " ".join(f"{k}={describe(v)}" for k, v in kw.items()))
    if cache is not None:
        kw.update(past_key_values=cache, use_cache=True)
    o = warned(lambda: m(x, **kw))
    o = o[0] if o is not None else None
    log(f"  out {describe(o)}")
    log(f"  mixing_matrix.data {describe(m.mixing_matrix.data)}")
    log_cache(cache)
    return o


def log_grads(tag, m, x, o, seed=5):
    if o is None:
        return
    dY = torch.randn(o.shape, generator=torch.Generator().manual_seed(seed)).to(o)
    (o * dY).sum().backward()
    log(f"grad {tag} x {describe(x.grad)}")
    for name, p in m.named_parameters():
        if SKIP_CONV_GRADS and name.endswith("_conv1d.weight"):
            continue
        log(f"grad {tag} {name} {describe(p.grad) if p.grad is not None else None}")
    m.zero_grad(set_to_none=True)


def make_layer(dtype, hidden=128, **kw):
    torch.manual_seed(3)
    m = fla.MHLA(**{**dict(mode="chunk", hidden_size=hidden, expand_k=0.5, expand_v=1.0, num_heads=2, feature_map="relu", norm_eps=1e-6), **kw})
    with torch.no_grad():
        (m.g_norm_swish_gate if m.fuse_norm_and_gate else m.g_norm).weight.uniform_(0.5, 1.5)
        m.mixing_matrix.copy_((1.2 * torch.rand(32, 32) - 0.1).view(32, 32, 1, 1, 1, 1))   # (some entries outside the clamp's range)
    return m.to(DEV).to(dtype)


def inputs(B, T, dtype, hidden=128, seed=11, grad=False):
    x = torch.randn(B, T, hidden, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)
    return x.requires_grad_(True) if grad else x


def left_mask(lengths, T):
    m = torch.zeros(len(lengths), T, dtype=torch.long)
    for b, n in enumerate(lengths):
        m[b, T - n:] = 1
    return m.to(DEV)


def cu_of(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32, device=DEV)


def reference_cases(dt, d):
    for T in (40, 64, 65, 200):
        m = make_layer(dt)
        x = inputs(2, T, dt, grad=True)
        log_grads(f"ref T={T} {d}", m, x, layer_call(f"ref T={T} {d}", m, x))
    options = [dict(fuse_norm=False), dict(use_output_gate=False), dict(gate_fn="sigmoid"), dict(num_kv_heads=1), dict(use_short_conv=True),
               dict(feature_map="elu"), dict(feature_map="identity"), dict(expand_k=0.3125)]   # (the last: head_k_dim = 20, eager rotary)
    for opts in options:
        for T in (40, 200):
            tag = f"ref {opts} T={T} {d}"
            m = make_layer(dt, **opts)
            x = inputs(2, T, dt, grad=True)
            log_grads(tag, m, x, layer_call(tag, m, x))
    for lengths, T in (((100, 37, 64), 100), ((20, 7, 30), 30), ((40, 37, 30), 40)):   # (the last: 107 packed tokens from a call of <= 64)
        m = make_layer(dt)
        x = inputs(3, T, dt, grad=True)
        tag = f"ref mask {lengths} {d}"
        log_grads(tag, m, x, layer_call(tag, m, x, attention_mask=left_mask(lengths, T)))
        xp = inputs(1, sum(lengths), dt, grad=True)
        tag = f"ref cu_seqlens {lengths} {d}"
        log_grads(tag, m, xp, layer_call(tag, m, xp, cu_seqlens=cu_of(lengths)))
    m = make_layer(dt, use_short_conv=True)
    xp = inputs(1, 201, dt, grad=True)
    log_grads(f"ref conv cu_seqlens {d}", m, xp, layer_call(f"ref conv cu_seqlens {d}", m, xp, cu_seqlens=cu_of((100, 37, 64))))
    # a non-exact cache: a masked 40-token call, then a masked one-token call (per-sequence rotary offsets)
    for opts in ({}, dict(use_short_conv=True)):
        m = make_layer(dt, layer_idx=0, **opts).eval()
        cache = fla.DecodeCache()
        total = torch.tensor([40, 7, 25])
        with torch.no_grad():
            mask = (torch.arange(40)[None, :] >= 40 - total[:, None]).long().to(DEV)
            layer_call(f"ref cache {opts} 40 {d}", m, inputs(3, 40, dt), cache, attention_mask=mask)
            mask = torch.cat([mask, torch.ones(3, 1, dtype=torch.long, device=DEV)], 1)
            layer_call(f"ref cache {opts} +1 {d}", m, inputs(3, 1, dt, seed=12), cache, attention_mask=mask)
            layer_call(f"ref cache {opts} +1 no mask {d}", m, inputs(3, 1, dt, seed=13), cache)


def isolate_cases(dt, d):
    for opts in ({}, dict(fuse_norm=False), dict(use_short_conv=True)):
        for lengths, T in (((100, 37, 64), 100), ((20, 7, 30), 30)):
            m = make_layer(dt, isolate_sequences=True, **opts)
            xp = inputs(1, sum(lengths), dt, grad=True)
            tag = f"iso {opts} cu_seqlens {lengths} {d}"
            log_grads(tag, m, xp, layer_call(tag, m, xp, cu_seqlens=cu_of(lengths)))
            x = inputs(3, T, dt, grad=True)
            tag = f"iso {opts} mask {lengths} {d}"
            log_grads(tag, m, x, layer_call(tag, m, x, attention_mask=left_mask(lengths, T)))
            plan = fla.causal_varlen_plan(cu_of(lengths), DEV)
            tag = f"iso {opts} plan {lengths} {d}"
            log_grads(tag, m, xp, layer_call(tag, m, xp, cu_seqlens=cu_of(lengths), varlen_plan=plan))
    m = make_layer(dt, isolate_sequences=True)
    x = inputs(2, 200, dt, grad=True)
    log_grads(f"iso plain {d}", m, x, layer_call(f"iso plain {d}", m, x))


def exact_uniform_cases(dt, d):
    for opts in ({}, dict(fuse_norm=False), dict(num_kv_heads=1), dict(use_short_conv=True)):
        for T0 in (1, 63, 64, 100):
            m = make_layer(dt, layer_idx=0, exact_decoding=True, **opts).eval()
            cache = fla.DecodeCache()
            x = inputs(2, T0 + 3 + 5 + 70, dt)
            at = 0
            with torch.no_grad():
                for n in (T0, 1, 1, 1, 5, 70):
                    layer_call(f"exact {opts} T0={T0} +{n} {d}", m, x[:, at:at + n], cache)
                    at += n
    m = make_layer(dt, layer_idx=0, exact_decoding=True).eval()
    cache = fla.DecodeCache()
    with torch.no_grad():   # an all-ones mask is no padding: a uniform state
        layer_call(f"exact ones-mask prefill {d}", m, inputs(2, 70, dt), cache, attention_mask=torch.ones(2, 70, dtype=torch.long, device=DEV))
        layer_call(f"exact ones-mask step {d}", m, inputs(2, 1, dt), cache, attention_mask=torch.ones(2, 71, dtype=torch.long, device=DEV))


def exact_ragged_cases(dt, d):
    for opts in ({}, dict(fuse_norm=False), dict(num_kv_heads=1)):
        m = make_layer(dt, layer_idx=0, exact_decoding=True, **opts).eval()
        cache = fla.DecodeCache()
        x = inputs(3, 100 + 2 + 5 + 5 + 1, dt)
        with torch.no_grad():
            layer_call(f"ragged {opts} prefill {d}", m, x[:, :100], cache, attention_mask=left_mask((100, 37, 64), 100))
            layer_call(f"ragged {opts} step {d}", m, x[:, 100:101], cache)
            layer_call(f"ragged {opts} step {d}", m, x[:, 101:102], cache)
            layer_call(f"ragged {opts} extend 5 {d}", m, x[:, 102:107], cache)
            layer_call(f"ragged {opts} counts {d}", m, x[:, 107:112], cache, token_counts=(1, 0, 5))
            layer_call(f"ragged {opts} counts tensor {d}", m, x[:, 107:112], cache, token_counts=torch.tensor([2, 5, 0]))
            layer_call(f"ragged {opts} ones mask {d}", m, x[:, 112:113], cache, attention_mask=torch.ones(3, 113, dtype=torch.long, device=DEV))
    m = make_layer(dt, layer_idx=0, exact_decoding=True).eval()   # a short padded prefill (<= 64 tokens: the unfused composition)
    cache = fla.DecodeCache()
    with torch.no_grad():
        layer_call(f"ragged short prefill {d}", m, inputs(3, 30, dt), cache, attention_mask=left_mask((30, 7, 12), 30))
        layer_call(f"ragged short step {d}", m, inputs(3, 1, dt), cache)


def device_position_cases(dt, d):
    for opts in ({}, dict(fuse_norm=False), dict(num_kv_heads=1)):
        for mask in (None, left_mask((60, 37), 60)):
            m = make_layer(dt, layer_idx=0, exact_decoding=True, **opts).eval()
            cache = fla.DecodeCache(device_positions=True)
            x = inputs(2, 63, dt)
            tag = f"dev {opts} {'padded' if mask is not None else 'uniform'} {d}"
            with torch.no_grad():
                layer_call(f"{tag} prefill", m, x[:, :60], cache, **({} if mask is None else {"attention_mask": mask}))
                for i in range(3):
                    layer_call(f"{tag} step {i}", m, x[:, 60 + i:61 + i], cache)
                cache.sync()
                log(f"{tag} after sync")
                log_cache(cache)


def gpt_cases(dt, d):
    def model(**kw):
        torch.manual_seed(4)
        return host.GPT_MHLA(vocab_size=97, hidden_size=128, num_layers=2, num_heads=2, max_seq_len=2048, **kw).to(DEV).to(dt)

    def call(tag, gpt, ids, cache=None, **kw):
        log(f"gpt {tag} ids={describe(ids)} " + " ".join(f"{k}={describe(v)}" for k, v in kw.items()))
        out = warned(lambda: gpt(ids, cache=cache, **kw))
        log(f"  gpt out {describe(out)}")
        log_cache(cache)
        return out
    gen = torch.Generator().manual_seed(6)
    ids = torch.randint(0, 97, (2, 212), generator=gen).to(DEV)
    gpt = model()
    loss = call(f"labels {d}", gpt, ids[:, :200], labels=ids[:, :200])
    loss.backward() if loss is not None else None
    for name, p in gpt.named_parameters():
        log(f"grad gpt labels {d} {name} {describe(p.grad) if p.grad is not None else None}")
    gpt = model(exact_decoding=True).eval()
    with torch.no_grad():
        cache = fla.DecodeCache()
        call(f"cache prefill {d}", gpt, ids[:, :100], cache)
        call(f"cache step {d}", gpt, ids[:, 100:101], cache)
        call(f"cache extend {d}", gpt, ids[:, 101:108], cache)
        cache = fla.DecodeCache()
        call(f"cache masked prefill {d}", gpt, ids[:, :100], cache, attention_mask=left_mask((100, 37), 100))
        call(f"cache ragged step {d}", gpt, ids[:, 100:101], cache)
        call(f"cache counts {d}", gpt, ids[:, 101:106], cache, token_counts=[1, 5])
        call(f"cache counts tensor {d}", gpt, ids[:, 106:111], cache, token_counts=torch.tensor([0, 3]))
        log(f"gpt generate {d} {describe(gpt.generate(ids[:, :20], 4, attention_mask=left_mask((20, 9), 20)))}")
    gpt = model(isolate_sequences=True).eval()
    with torch.no_grad():
        call(f"iso cu_seqlens {d}", gpt, ids[:1, :137], cu_seqlens=cu_of((37, 100)))
        call(f"iso mask {d}", gpt, ids[:, :100], attention_mask=left_mask((37, 100), 100))
    gpt = model().eval()
    with torch.no_grad():
        call(f"plain cu_seqlens {d}", gpt, ids[:1, :137], cu_seqlens=cu_of((37, 100)))
        call(f"plain mask {d}", gpt, ids[:, :100], attention_mask=left_mask((37, 100), 100))


def main():
    global SKIP_CONV_GRADS
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--no-conv-grads", action="store_true", help="leave the gradient lines of *_conv1d.weight out")
    a = ap.parse_args()
    SKIP_CONV_GRADS = a.no_conv_grads
    for name in SPIED:
        setattr(fla, name, spy(name, getattr(fla, name)))
    for dt, d in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        for cases in (reference_cases, isolate_cases, exact_uniform_cases, exact_ragged_cases, device_position_cases, gpt_cases):
            cases(dt, d)
            print(f"{cases.__name__} {d}: {len(LOG)} lines", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LOG) + "\n")
    print(f"{len(LOG)} lines, sha256 {hashlib.sha256(chr(10).join(LOG).encode()).hexdigest()} -> {a.out}")


if __name__ == "__main__":
    main()
