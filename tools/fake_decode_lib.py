"""A stand-in for libmhla_hip.so that records the library calls of `mhla_amd.ops` instead of launching them, so that a host layer
(checks, slicing, marshalling) runs on CPU tensors, without a GPU.  It began with the decode section and serves every section of
`ops.py` whose nodes are Python: used by tools/record_decode_calls.py and tests/test_decode_calls_cpu.py (causal decode) and by
tools/record_blockmix_calls.py and tests/test_blockmix_calls_cpu.py (block-mix operators, LePE, rotary and q / k prologues).

    with Session(ops, _lib) as s:
        s.name(q=q, k=k, v=v, mix=mix, S=state.S, P=state.P, Cur=state.Cur, pos=state.pos)
        s.call("step", ops.mhla_causal_step, q, k, v, mix, state, state=state)
    s.calls   # [Call(name, args)], s.lines: the same as text

Inside the `with`, `ops._require_gpu` and `ops._stream` are stubs and `_lib.load()` returns the recorder: every launching entry point
is logged and returns 0 -- whatever `_lib.SIGNATURES` names, the slotted (`mhla_causal_*_slots`) and the paged calls among them
(`mhla_causal_step_paged`, `mhla_causal_step_dev_paged`, `mhla_causal_extend_paged`, `mhla_causal_verify_paged`,
`mhla_causal_commit_paged`, `mhla_causal_varlen_state_init_paged`: name `pages` and `table_dev` to see them in a call; on h16 pages
`mhla_causal_step_paged_h16`, `mhla_causal_step_dev_paged_h16` and `mhla_causal_varlen_state_init_paged_h16`, which take the payload
and `page_mult` where those take `pages`, the prefill a workspace too) --; the entry points that are host arithmetic (`*_ws_bytes`, `*_keeps_state`, `*_ok`, `*_dw_rows`, `*_fusable`,
the two `describe` calls, `mhla_set_option`, `mhla_abi_version`, `mhla_build_flags`) go to the real library, and the text log
(`lines`, not `calls`) shows each with its integer arguments and its result.  An argument is recorded by its C type:
a view as ("view", base, element offset, sb, sn, sh), a pointer as ("ptr", base, byte offset), a workspace as ("ws", bytes), a null
as ("null",), a scalar as itself.  `base` is the name a tensor was given with `name()`; storage allocated inside the call is named
"new<n>" in order of allocation (a dispatch mode sees every allocation and keeps it alive until the call returns, so that no
address is used twice)."""
import ctypes
from collections import namedtuple

import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_leaves

Call = namedtuple("Call", "name args")


def batch_of(call: Call) -> int:
    """B of a recorded decode call: the integer after the workspace and its size in every decode entry point."""
    i = next(i for i, a in enumerate(call.args) if isinstance(a, tuple) and a[0] == "ws")
    return call.args[i + 1]


class _Allocations(TorchDispatchMode):
    def __init__(self, session):
        super().__init__()
        self.session = session

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        for t in tree_leaves(out):
            if isinstance(t, torch.Tensor):
                self.session._allocated(t)
        return out


# entry points that launch nothing: answered by the real library
_HOST_SUFFIXES = ("_ws_bytes", "_keeps_state", "_ok", "_dw_rows", "_fusable")
_HOST_NAMES = ("mhla_describe_dispatch", "mhla_causal_describe_dispatch", "mhla_set_option", "mhla_abi_version", "mhla_build_flags")


class _Recorder:
    """What `_lib.load()` returns inside a Session."""

    def __init__(self, session, real):
        self._session, self._real = session, real

    def __getattr__(self, name):
        if name.startswith("__") or name not in self._session.lib_mod.SIGNATURES:
            raise AttributeError(name)
        if name == "mhla_last_error":
            return getattr(self._real, name)
        if name.endswith(_HOST_SUFFIXES) or name in _HOST_NAMES:
            return lambda *args: self._session._passed_through(name, args, getattr(self._real, name)(*args))
        return lambda *args: self._session._record(name, args)


class Session:
    def __init__(self, ops, lib_mod):
        self.ops, self.lib_mod = ops, lib_mod
        self.calls, self.lines = [], []
        self._named, self._new = [], []

    def __enter__(self):
        real = self.lib_mod.load()
        self._saved = (self.ops._require_gpu, self.ops._stream, self.lib_mod.load)
        recorder = _Recorder(self, real)
        self.ops._require_gpu = lambda *ts: None
        self.ops._stream = lambda: 0
        self.lib_mod.load = lambda: recorder
        return self

    def __exit__(self, *exc):
        self.ops._require_gpu, self.ops._stream, self.lib_mod.load = self._saved

    # ---- naming storage
    @staticmethod
    def _range(t):
        st = t.untyped_storage()
        return st.data_ptr(), st.nbytes(), t.element_size()

    def name(self, **tensors):
        """Give the storage of every tensor a name (a view and its base share one: name the base)."""
        for label, t in tensors.items():
            if t is not None:
                self._named = [e for e in self._named if e[0] != label] + [(label, *self._range(t), t)]

    def _find(self, ptr):
        for label, lo, n, size, _ in self._named + self._new:
            if lo <= ptr < lo + max(n, 1):
                return label, ptr - lo, size
        return None

    def _allocated(self, t):
        lo, n, size = self._range(t)
        if n and self._find(lo) is None:
            self._new.append((f"new{len(self._new)}", lo, n, size, t))

    # ---- recording
    def _pointer(self, ptr):
        if not ptr:
            return ("null",)
        hit = self._find(ptr)
        return ("ptr", "?", 0) if hit is None else ("ptr", hit[0], hit[1])

    def _record(self, name, args):
        types = self.lib_mod.SIGNATURES[name][1]
        assert len(types) == len(args), f"{name}: {len(args)} arguments for {len(types)} parameters"
        out, i = [], 0
        while i < len(args):
            a, ty = args[i], types[i]
            if ty is self.lib_mod.View:
                if not a.ptr:
                    out.append(("null",))
                else:
                    hit = self._find(a.ptr) or ("?", 0, 1)
                    assert hit[1] % hit[2] == 0
                    out.append(("view", hit[0], hit[1] // hit[2], a.sb, a.sn, a.sh))
            elif ty is ctypes.c_void_p and i + 1 < len(types) and types[i + 1] is ctypes.c_size_t:
                out.append(("ws", int(args[i + 1])))
                i += 1
            elif ty is ctypes.c_void_p and i == len(args) - 1:
                out.append(("stream", a))
            elif ty is ctypes.c_void_p:
                out.append(self._pointer(a))
            else:
                out.append(a)
            i += 1
        self.calls.append(Call(name, tuple(out)))
        self.lines.append(f"  {name}({', '.join(map(repr, out))})")
        return 0

    def _passed_through(self, name, args, result):
        shown = ", ".join(repr(a) if isinstance(a, (int, float, bytes)) else "buffer" for a in args)
        self.lines.append(f"  {name}({shown}) = {result!r}")
        return result

    def call(self, label, fn, *args, state=None, catch=True, **kw):
        """Run one public call: its library calls, then its result (shape and base), or the exception's type and message, then
        what it left in `state`'s host mirror.  Returns the result (None after an exception; `catch=False` lets it through)."""
        self.lines.append(f"{label}:")
        self._new = []
        result = None
        try:
            with _Allocations(self):
                result = fn(*args, **kw)
        except Exception as e:   # noqa: BLE001
            if not catch:
                raise
            self.lines.append(f"  raised {type(e).__name__}: {e}")
        else:
            for r in (result if isinstance(result, tuple) else (result,)):
                if isinstance(r, torch.Tensor):
                    hit = self._find(r.data_ptr()) or ("?", 0, 1)
                    self.lines.append(f"  returned {tuple(r.shape)} {r.dtype} strides {r.stride()} in {hit[0]}+{hit[1]}")
                else:
                    self.lines.append(f"  returned {r!r}")
        if state is not None:
            pos = None if state.pos is None else state.pos.tolist()
            self.lines.append(f"  state: seen={state.seen} lengths={state.lengths} stale={state.stale} pos={pos}")
        self._new = []
        return result
