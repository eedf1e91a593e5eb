"""The device-positioned decode step as far as a machine without a GPU reaches it: `CausalState.to_ragged` / `full` / `sync`, the
refusal of a stale host mirror by the calls that read it, the checks `mhla_causal_step_dev` makes before it touches a device (in
their order), and the C-ABI symbol with its static argument checks.  The kernels are in tests/test_gpu_causal_step_dev.py."""
import pytest
import torch

import mhla_amd
from mhla_amd import CausalState

B, H, K, V, CAP = 2, 3, 16, 24, 5


def _ragged(lengths=(7, 70), k=K, cap=CAP):
    e = CausalState.empty(len(lengths), H, k, V, cap, device="cpu")
    return CausalState(e.S, e.P, e.Cur, 0, 64, lengths=lengths)


def test_to_ragged_shares_the_storage():
    u = CausalState.empty(B, H, K, V, CAP, device="cpu")
    u.seen = 9
    r = u.to_ragged()
    assert r is not u and r.lengths == (9, 9) and r.seen == 9 and r.pos.tolist() == [9, 9] and r.pos.dtype == torch.int32
    assert all(getattr(r, n).data_ptr() == getattr(u, n).data_ptr() for n in ("S", "P", "Cur"))
    assert r.to_ragged() is r and u.lengths is None and not r.stale and not u.stale


def test_full_is_created_on_first_use_and_carried():
    st = _ragged()
    base = 4 * (st.S.numel() + st.P.numel() + st.Cur.numel() + 2)
    assert st.nbytes == base                                  # (not created yet: a state that never takes the path pays nothing)
    f = st.full
    assert f.dtype == torch.int32 and f.tolist() == [0, 0] and f.device == st.S.device and st.full is f
    assert st.nbytes == base + 8
    f[1] = 1
    c = st.clone()
    assert c.full.tolist() == [0, 1] and c.full.data_ptr() != f.data_ptr()
    both = CausalState.cat([st, _ragged((3,))])
    assert both.full.tolist() == [0, 1, 0] and both.lengths == (7, 70, 3)
    assert CausalState.cat([_ragged((3,)), _ragged((4,))]).nbytes == 4 * (2 * (CAP + 2) * H * K * V + 2)   # (none had one: none made)


def test_sync_reads_the_device_side_back():
    st = _ragged()
    st.pos += 3          # what three device-positioned steps leave: the array ahead of the mirror
    st.stale = True
    assert st.lengths == (7, 70)
    assert st.sync() is st and st.lengths == (10, 73) and st.seen == 73 and not st.stale
    st.pos += 1
    st.full[0] = 1
    st.stale = True
    with pytest.raises(IndexError, match=r"sequences \[0\]") as info:
        st.sync()
    assert "capacity" in str(info.value)
    assert st.lengths == (11, 74) and st.seen == 74 and not st.stale      # the mirror was refreshed before the report
    u = CausalState.empty(B, H, K, V, CAP, device="cpu")
    assert u.sync() is u and u.lengths is None


def test_a_stale_mirror_is_refused_by_the_calls_that_read_it():
    st = _ragged()
    st.stale = True
    mix = torch.ones(CAP, CAP)
    tok = lambda T: (torch.zeros(B, T, H, K), torch.zeros(B, T, H, K), torch.zeros(B, T, H, V))
    for name, T in (("mhla_causal_step", 1), ("mhla_causal_extend", 5)):
        with pytest.raises(ValueError, match=r"sync\(\)") as info:
            getattr(mhla_amd, name)(*tok(T), mix, st)
        assert name in str(info.value)
    with pytest.raises(ValueError, match=r"CausalState.cat.*sync\(\)"):
        CausalState.cat([_ragged((1,)), st])
    assert st.clone().stale
    st.sync()
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # in step with the device again: the call goes on to the device check
        mhla_amd.mhla_causal_step(*tok(1), mix, st)


def _raises(exc, match, *args, **kw):
    with pytest.raises(exc, match=match) as info:
        mhla_amd.mhla_causal_step_dev(*args, **kw)
    assert type(info.value) is exc, f"{type(info.value).__name__}, expected {exc.__name__}"
    assert "mhla_causal_step_dev" in str(info.value) or match in (None, "no CPU fallback")
    return str(info.value)


def test_validation_order_and_messages():
    k8 = 16
    st = _ragged()
    mix = torch.ones(CAP, CAP)
    q, k, v = torch.zeros(B, 1, H, k8), torch.zeros(B, 1, H, k8), torch.zeros(B, 1, H, V)
    cos, sin = torch.zeros(64 * CAP, k8 // 2), torch.zeros(64 * CAP, k8 // 2)
    _raises(RuntimeError, "no CPU fallback", q, k, v, mix, st, feature_map="relu", rotary=(cos, sin))   # everything in order: the device check
    _raises(TypeError, "must be a CausalState", q, k, v, mix, (st.S, st.P, st.Cur))
    _raises(ValueError, None, q[0], k, v, mix, st)
    _raises(ValueError, "one token per call", *(torch.zeros(B, 2, H, d) for d in (k8, k8, V)), mix, st)
    uni = CausalState.empty(B, H, k8, V, CAP, device="cpu")
    assert "to_ragged()" in _raises(ValueError, "uniform", q, k, v, mix, uni)
    # the matrix is bounded by the capacity, not by the current length: one row or one column short is refused
    _raises(IndexError, "capacity of 5 chunks", q, k, v, torch.ones(CAP - 1, CAP), st)
    _raises(IndexError, "capacity of 5 chunks", q, k, v, torch.ones(CAP, CAP - 1), st)
    msg = _raises(ValueError, "at least 320 rows", q, k, v, mix, st, rotary=(cos[:-1], sin[:-1]))
    assert "cos" in msg
    _raises(ValueError, "rotary sin is torch.bfloat16", q, k, v, mix, st, rotary=(cos, sin.bfloat16()))
    _raises(ValueError, "K/2=8 entries per row", q, k, v, mix, st, rotary=(cos[:, :4], sin[:, :4]))
    q20, k20 = torch.zeros(B, 1, H, 20), torch.zeros(B, 1, H, 20)
    st20 = _ragged(k=20)
    _raises(ValueError, "K % 8 == 0", q20, k20, v, mix, st20, rotary=(torch.zeros(320, 10), torch.zeros(320, 10)))
    _raises(ValueError, "K % 8 == 0", q20, k20, v, mix, st20, feature_map="relu")
    _raises(RuntimeError, "no CPU fallback", q20, k20, v, mix, st20)            # (no prologue: any K % 4 == 0)
    _raises(ValueError, "feature_map 'gelu'", q, k, v, mix, st, feature_map="gelu")
    # order: the state's kind before the matrix, the matrix before the tables, the tables before the feature map; then the
    # checks shared with mhla_causal_step, in its order
    _raises(ValueError, "uniform", q, k, v, torch.ones(2, 2), uni, rotary=(cos[:1], sin[:1]))
    _raises(IndexError, "capacity", q, k, v, torch.ones(2, 2), st, rotary=(cos[:1], sin[:1]), feature_map="gelu")
    _raises(ValueError, "at least 320 rows", q, k, v, mix, st, rotary=(cos[:1], sin[:1]), feature_map="gelu")
    _raises(ValueError, "feature_map 'gelu'", q, k, v[:, :, :2], mix, st, feature_map="gelu")
    _raises(ValueError, "v has shape", q, k, v[:, :, :2], mix, st)
    _raises(ValueError, "k has dtype", q, k.bfloat16(), v, mix, st)
    _raises(ValueError, "norm_weight has 25 entries", q.clone().requires_grad_(), k, v, mix, st, norm_weight=torch.ones(V + 1))
    _raises(RuntimeError, "inference only", q.clone().requires_grad_(), k, v, mix, st)
    # nothing was touched, nothing marked stale by a refused call
    assert st.lengths == (7, 70) and st.pos.tolist() == [7, 70] and not st.stale and float(st.Cur.abs().max()) == 0.0
    # a stale mirror is no obstacle here: the call reads no host position
    st.stale = True
    _raises(RuntimeError, "no CPU fallback", q, k, v, mix, st)


def test_dev_entry_point_is_exported_at_abi_9():
    from mhla_amd import build as b, _lib
    b.build()
    lib = _lib.load()
    assert "mhla_causal_step_dev" in _lib.SIGNATURES and callable(lib.mhla_causal_step_dev)
    assert lib.mhla_abi_version() == _lib.ABI_VERSION == 9
    nv = _lib.NULL_VIEW
    # every argument check is host arithmetic, made before anything touches a device.  The addresses below are made up and never
    # dereferenced on the host; every case has a second, independent reason to be refused -- a null workspace, the last check
    # before the launches -- so that no loosening of one check can launch on them.
    fake = lambda: _lib.View(0x10000, 64, 64, 16)

    def raw(ldmix=2, cap=2, pos=0x10000, full=0x10000, cos=None, sin=None, ld_tab=0, rows=0, fmap=0, K=8):
        return lib.mhla_causal_step_dev(fake(), fake(), fake(), 0x10000, ldmix, 0x10000, cap, 0x10000, 0x10000, pos, full, cos, sin, ld_tab,
                                        rows, fmap, fake(), nv, None, 1e-5, nv, None, 0, 1, 1, K, 4, 64, 1.0, _lib.F32, None)
    err = lambda: lib.mhla_last_error()
    assert raw() == -22 and b"workspace too small" in err()                      # (the second reason, on its own)
    assert raw(cos=0x10000, sin=0x10000, ld_tab=4, rows=128, fmap=2) == -22 and b"workspace too small" in err()
    assert raw(ldmix=1) == -22 and b"cap_chunks=2" in err() and b"row 1" in err()
    assert raw(pos=None) == -22 and b"pos_dev" in err()
    assert raw(full=None) == -22 and b"full_dev" in err()
    assert raw(cos=0x10000) == -22 and b"together" in err()
    assert raw(sin=0x10000) == -22 and b"together" in err()
    assert raw(cos=0x10000, sin=0x10000, ld_tab=4, rows=127) == -22 and b"tab_rows=127" in err()
    assert raw(cos=0x10000, sin=0x10000, ld_tab=2, rows=128) == -22 and b"ld_tab" in err()
    assert raw(cos=0x10000, sin=0x10000, ld_tab=6, rows=128) == -22 and b"ld_tab" in err()
    assert raw(cos=0x10004, sin=0x10000, ld_tab=4, rows=128) == -22 and b"aligned" in err()
    assert raw(cos=0x10000, sin=0x10000, ld_tab=4, rows=128, K=12) == -22 and b"K=12" in err()
    assert raw(fmap=1, K=12) == -22 and b"K=12" in err()
    assert raw(K=12) == -22 and b"workspace too small" in err()                  # (no prologue: K % 4 == 0 is enough)
    assert raw(fmap=3) == -22 and b"feature_map 3" in err()
