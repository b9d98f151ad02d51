"""torch.autograd.Function wrappers over the C ABI (include/mvdseg_hip.h).

PyTorch supplies device memory (caching allocator), the current HIP stream and the autograd tape; every
arithmetic operation of the hot path runs in libmvdseg_hip.so.  Activations are 5-D tensors of logical shape
[N,C,D,H,W] stored NDHWC (torch.channels_last_3d); logits / targets / volumes of the topology losses are planar.
"""
import ctypes
import functools
import os
import time
import typing
import weakref

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import call, i3, query

CL3D = torch.channels_last_3d


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("multimodal_mvd_seg_amd ops need tensors on the MI355X (cuda) device; "
                               "there is no CPU fallback")
        if t is not None and t.dtype not in (torch.float32, torch.bfloat16, torch.uint8, torch.int32, torch.int64,
                                             torch.int16):
            raise RuntimeError(f"unsupported dtype {t.dtype} (kernels take fp32, or bf16 activations in mixed precision)")


class _Workspace:
    """Grow-only scratch buffer per device; kernels of one stream run in order so sharing it is safe."""
    _bufs = {}

    @classmethod
    def get(cls, nbytes, device):
        key = (device.index, torch.cuda.current_stream().cuda_stream)
        buf = cls._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
            cls._bufs[key] = buf
        return buf


def _take_grad(param):
    """Direct gradient sink of optim.FlatParams: the tensor to write this parameter's gradient into (its slice of the
    flat gradient buffer) when it has not been written in this step, else None (-> return the gradient to autograd)."""
    take = getattr(param, '_mvd_take_grad', None) if param is not None else None
    t = take() if take is not None else None
    if t is not None and not (t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda):
        raise RuntimeError("flat gradient slice must be a contiguous fp32 cuda tensor")
    return t


def _grad_done(param):
    done = getattr(param, '_mvd_grad_done', None)
    if done is not None:
        done()


def ks3(weight):
    """Kernel size of a conv weight as three axes: a 2-D layer's [K,C,kh,kw] parameter is the [K,C,1,kh,kw] weight of the
    same memory (the 2-D modules of network.py pass their real parameters, so that the packed-weight cache, the flat
    gradient slices and the fused optimizer see the parameter itself)."""
    sp = tuple(weight.shape[2:])
    return (1,) + sp if len(sp) == 2 else sp


def _is_cl3d(t):
    return t.dim() == 5 and t.is_contiguous(memory_format=CL3D)


def empty_cl3d(shape, device, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=device, memory_format=CL3D)


BF16 = torch.bfloat16


def _is_bf16(t):
    return t is not None and t.dtype == BF16


def to_ndhwc(t):
    """[N,C,D,H,W] in any layout -> physical NDHWC (HIP transpose kernel when the tensor is planar)."""
    _require_cuda(t)
    if _is_cl3d(t):
        return t
    if t.dtype == BF16:
        # bf16 activations are produced NDHWC by these ops; a planar one can only come from outside the path
        raise RuntimeError("bf16 activations must already be NDHWC (torch.channels_last_3d)")
    if not t.is_contiguous():
        t = t.contiguous()
    N, C = t.shape[:2]
    V = t[0, 0].numel()
    out = empty_cl3d(t.shape, t.device)
    call("mvd_nchw_to_ndhwc", _p(t), _p(out), N, C, V, _stream())
    return out


def to_planar(t):
    """physical NDHWC -> contiguous NCDHW."""
    _require_cuda(t)
    if t.is_contiguous():
        return t
    if not _is_cl3d(t):
        return t.contiguous()
    N, C = t.shape[:2]
    V = t[0, 0].numel()
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    call("mvd_ndhwc_to_nchw", _p(t), _p(out), N, C, V, _stream())
    return out


def pack_weight(weight, transposed):
    """torch Conv3d [K,C,kd,kh,kw] / ConvTranspose3d [C,K,kd,kh,kw] -> (wf [T,C,K], wb [T,K,C])."""
    w = weight.detach()
    if not w.is_contiguous():
        w = w.contiguous()
    if transposed:
        C, K = w.shape[:2]
    else:
        K, C = w.shape[:2]
    T = w[0, 0].numel()
    wf = torch.empty((T, C, K), dtype=torch.float32, device=w.device)
    wb = torch.empty((T, K, C), dtype=torch.float32, device=w.device)
    call("mvd_pack_weight", _p(w), _p(wf), _p(wb), K, C, T, 1 if transposed else 0, _stream())
    return wf, wb


# ---------------------------------------------------------------------------------------------- packed-weight cache (fp32)
# The packed copies (wf / wb, Winograd uf / ub) of a conv weight live on the weight tensor object (`_mvd_pack`) and are
# valid for one stamp = (global pack epoch, epoch of the flat buffer the parameter is a view of, version of the parameter,
# storage pointer, version of that flat buffer).  torch in-place writes to the parameter or to optim.FlatParams.flat
# (dist.broadcast, `flat -= ...`) bump a version; the fused optimizer -- which updates ITS flat buffer through a raw
# pointer -- bumps that buffer's epoch and re-packs the weights that live in it in ONE launch (repack_all(fp):
# mvd_pack_weights_batch3); the weights of another optimizer in the process are not touched (round 3: they used to be
# re-packed and their saved graphs invalidated too).  A stale or missing entry is packed on the spot by the per-layer
# entries.  The one write torch cannot see is `p.data.copy_()` / any other raw-pointer writer: such code must call
# invalidate_packs() (FlatParams.invalidate_packs), which bumps the global epoch.
_PACK_EPOCH = [0]
_PACK_LIVE = []
_PACK16_LIVE = []
_PACK16PAD_LIVE = []   # weights carrying the zero-padded pack of the narrow input conv (_mvd_pack16pad)


def invalidate_packs():
    """Declare every cached packed weight stale (after a write to parameter memory that bypasses torch's version
    counters).  The next forward re-packs per layer."""
    _PACK_EPOCH[0] += 1


def _check_pack_generation(saved, what):
    """`saved` = (entry, generation at forward time).  The fp32 packs are rebuilt IN PLACE; a graph kept across a weight
    update would silently back-propagate through the new weights (torch raises for its own saved tensors: so do we)."""
    if saved is not None and saved[0].gen != saved[1]:
        raise RuntimeError(f"{what}: the weights were updated (optimizer.step() or an in-place write) between the forward "
                           "and the backward pass of this graph; the packed copies saved for backward were rebuilt")


class _PackEntry:
    __slots__ = ("transposed", "K", "C", "T", "wf", "wb", "uf", "ub", "vf", "vb", "stamp", "gen")


def _flat_of(w, owner=None):
    return getattr(owner if owner is not None else w, "_mvd_flat", None)


def _pack_stamp(w, owner=None):
    # data_ptr: `p.data = other` swaps the storage without a version bump on the parameter object
    flat = _flat_of(w, owner)
    local = getattr(flat, "_mvd_epoch", None) if flat is not None else None
    return (_PACK_EPOCH[0], local[0] if local is not None else 0, w._version, w.data_ptr(),
            flat._version if flat is not None else -1)


def _packed(weight, transposed, want_uf=False, want_ub=False, want_vf=False, want_vb=False):
    """uf / ub: the F(2x2,3x3) tables (mvd_pack_weight_wino; of a 9-tap weight: those of the 1x3x3 engine,
    mvd_pack_weight_wino2p -- the caller asks for them for kernel size (1,3,3) only), vf / vb: the F(2x2x2,3x3x3) tables
    (mvd_pack_weight_wino3)."""
    w = weight.detach()
    sfx2 = "2p" if w[0, 0].numel() == 9 else ""
    if sfx2 and (want_uf or want_ub) and ks3(w) != (1, 3, 3):
        # (3,3,1) and (3,1,3) weights have 9 taps too; the 9-tap tables -- here and as the T = 9 job of the batched
        # repack, which packs whatever entry carries uf / ub -- are those of the in-plane kernel alone
        raise RuntimeError(f"_packed: Winograd tables of a 9-tap weight exist for kernel size (1,3,3) only, got {ks3(w)}")
    if not w.is_contiguous():  # no cache for a strided view: pack a contiguous copy
        e = _PackEntry()
        e.gen = 0
        e.wf, e.wb = pack_weight(weight, transposed)
        e.uf = e.ub = e.vf = e.vb = None
        wc = w.contiguous()
        K, C = wc.shape[:2]
        if want_uf or want_ub:
            n = query("mvd_wino%s_weight_elems" % sfx2, C, K)
            e.uf = torch.empty((n,), dtype=torch.float32, device=w.device) if want_uf else None
            e.ub = torch.empty((n,), dtype=torch.float32, device=w.device) if want_ub else None
            call("mvd_pack_weight_wino" + sfx2, _p(wc), _p(e.uf), _p(e.ub), K, C, _stream())
        if want_vf or want_vb:
            n = query("mvd_wino3_weight_elems", C, K)
            e.vf = torch.empty((n,), dtype=torch.float32, device=w.device) if want_vf else None
            e.vb = torch.empty((n,), dtype=torch.float32, device=w.device) if want_vb else None
            call("mvd_pack_weight_wino3", _p(wc), _p(e.vf), _p(e.vb), K, C, _stream())
        return e
    e = getattr(weight, "_mvd_pack", None)
    stale = False
    if e is None or e.transposed != transposed or e.wf.device != w.device:
        e = _PackEntry()
        e.transposed = transposed
        if transposed:
            e.C, e.K = w.shape[:2]
        else:
            e.K, e.C = w.shape[:2]
        e.T = w[0, 0].numel()
        e.wf = torch.empty((e.T, e.C, e.K), dtype=torch.float32, device=w.device)
        e.wb = torch.empty((e.T, e.K, e.C), dtype=torch.float32, device=w.device)
        e.uf = e.ub = e.vf = e.vb = None
        e.stamp = None
        e.gen = 0
        weight._mvd_pack = e
        if len(_PACK_LIVE) >= 4096:  # inference-only use never calls repack_all: drop dead references here
            _PACK_LIVE[:] = [r for r in _PACK_LIVE if r() is not None]
        _PACK_LIVE.append(weakref.ref(weight))
        stale = True
    new_wino = False
    if (want_uf and e.uf is None) or (want_ub and e.ub is None):
        n = query("mvd_wino%s_weight_elems" % sfx2, e.C, e.K)
        if want_uf and e.uf is None:
            e.uf = torch.empty((n,), dtype=torch.float32, device=w.device)
        if want_ub and e.ub is None:
            e.ub = torch.empty((n,), dtype=torch.float32, device=w.device)
        new_wino = True
    new_wino3 = False
    if (want_vf and e.vf is None) or (want_vb and e.vb is None):
        n = query("mvd_wino3_weight_elems", e.C, e.K)
        if want_vf and e.vf is None:
            e.vf = torch.empty((n,), dtype=torch.float32, device=w.device)
        if want_vb and e.vb is None:
            e.vb = torch.empty((n,), dtype=torch.float32, device=w.device)
        new_wino3 = True
    if stale or e.stamp != _pack_stamp(w, weight):
        e.gen += 1  # wf / wb / uf / ub / vf / vb are overwritten in place
        call("mvd_pack_weight", _p(w), _p(e.wf), _p(e.wb), e.K, e.C, e.T, 1 if transposed else 0, _stream())
        new_wino = e.uf is not None or e.ub is not None
        new_wino3 = e.vf is not None or e.vb is not None
        e.stamp = _pack_stamp(w, weight)
    if new_wino:
        call("mvd_pack_weight_wino" + sfx2, _p(w), _p(e.uf), _p(e.ub), e.K, e.C, _stream())
    if new_wino3:
        call("mvd_pack_weight_wino3", _p(w), _p(e.vf), _p(e.vb), e.K, e.C, _stream())
    return e


def _live(refs, attr, fp):
    """(weight, cache entry) of the live registered weights -- all of them, or those that are views of `fp`'s buffer."""
    out, alive = [], []
    for r in refs:
        w = r()
        e = getattr(w, attr, None) if w is not None else None
        if e is None:
            continue
        alive.append(r)
        if fp is None or _flat_of(w) is fp.flat:
            out.append((w, e))
    refs[:] = alive
    return out


def _pack16_launch(jobs, dev):
    """One mvd_pack_weights_bf16_batch_pad launch: jobs = (fp32 source, wf16, wb16, K, C, T, transposed, Csrc)."""
    n = len(jobs)
    PA, IA = ctypes.c_void_p * n, ctypes.c_int * n
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    col = lambda i: cast(IA(*[int(j[i]) for j in jobs]))
    with torch.cuda.device(dev):
        call("mvd_pack_weights_bf16_batch_pad", n, cast(PA(*[j[0].data_ptr() for j in jobs])),
             cast(PA(*[j[1].data_ptr() for j in jobs])), cast(PA(*[j[2].data_ptr() for j in jobs])),
             col(3), col(4), col(5), col(6), col(7), _stream())


class _Pack16(typing.NamedTuple):
    """A cached bf16 pack (`_mvd_pack16`: key = (stamp, transposed, device); `_mvd_pack16pad`: key = (stamp, padded reduce
    channels, device)).  inplace: wf / wb are views of the persistent buffer of a hipGraph trainer's FlatParams."""
    key: tuple
    wf: torch.Tensor
    wb: torch.Tensor
    inplace: bool = False


def _pack16_shape(d, transposed=False, cpad=None):
    """(K, C, T, transposed, Csrc) of the pack job of weight `d`; cpad: the conv weight packed as if it had cpad reduce
    channels, the ones beyond its own being zero."""
    if cpad is not None:
        return d.shape[0], int(cpad), d[0, 0].numel(), 0, d.shape[1]
    (C, K) = d.shape[:2] if transposed else (d.shape[1], d.shape[0])
    return K, C, d[0, 0].numel(), 1 if transposed else 0, C


def _pack16_rewrite(weight, e, shape):
    """A stale bf16 entry whose tensors are views of the persistent buffer of a hipGraph trainer (e.inplace): the captured
    forward reads THOSE addresses, so the on-the-spot pack writes into them (re-pointing the entry at fresh tensors would
    leave the replay on the old weights and every later eager forward on tensors no replay rewrites).  Only THIS weight's
    pack changes, so only its own generation moves: the guards other layers took earlier in the same forward stay valid."""
    d = weight.detach()
    _pack16_launch([(d, e.wf, e.wb) + shape], d.device)
    _pack16_own_gen(weight)[0] += 1
    return _Pack16((_pack_stamp(d, weight),) + e.key[1:], e.wf, e.wb, True)


def _repack_all_bf16(fp=None):
    """The bf16 packs of the live weights (of `fp`, or all) that have them -- the zero-padded pack of the input conv
    included -- in one launch (mvd_pack_weights_bf16_batch_pad) into views of ONE buffer per device.  Default: a FRESH
    buffer per call -- the tensors an autograd graph saved for backward keep their old buffer alive, exactly as with the
    per-layer packs (fresh tensors per stamp).  With `fp.pack16_inplace` (set by a trainer that replays its step as a
    hipGraph: the captured forward must read the addresses the captured repack of the previous replay wrote) the buffer is
    owned by `fp`, persists and is rewritten in place; `fp.pack16_gen` then guards saved autograd graphs the way the fp32
    entries' generations do."""
    jobs = []   # (weight data, weight, cache attribute, job shape)
    for w, e in _live(_PACK16_LIVE, "_mvd_pack16", fp):
        d = w.detach()
        if d.is_cuda and d.dtype == torch.float32 and d.is_contiguous() and d.device == e.key[2]:
            jobs.append((d, w, "_mvd_pack16", _pack16_shape(d, transposed=e.key[1])))
    for w, e in _live(_PACK16PAD_LIVE, "_mvd_pack16pad", fp):
        d = w.detach()
        if d.is_cuda and d.dtype == torch.float32 and d.is_contiguous() and d.device == e.key[2]:
            jobs.append((d, w, "_mvd_pack16pad", _pack16_shape(d, cpad=e.key[1])))
    inplace = fp is not None and getattr(fp, "pack16_inplace", False)
    for dev in {j[0].device for j in jobs}:
        js = [j for j in jobs if j[0].device == dev]
        sizes = [q[0] * q[1] * q[2] for _d, _w, _a, q in js]
        pad = lambda n: (n + 127) // 128 * 128  # 256-byte aligned views
        total = 2 * sum(pad(n) for n in sizes)
        buf = None
        if inplace:
            sig = (dev, tuple((id(w), attr, n) for (_d, w, attr, _q), n in zip(js, sizes)))
            held = getattr(fp, "_pack16_buf", None)
            if held is not None and held[0] == sig:
                buf = held[1]
                fp.pack16_gen[0] += 1
            else:
                buf = torch.empty((total,), dtype=BF16, device=dev)
                fp._pack16_buf = (sig, buf)
        if buf is None:
            buf = torch.empty((total,), dtype=BF16, device=dev)
        views, o = [], 0
        for n in sizes:
            views.append((buf[o:o + n], buf[o + pad(n):o + pad(n) + n]))
            o += 2 * pad(n)
        _pack16_launch([(d, v[0], v[1]) + q for (d, _w, _a, q), v in zip(js, views)], dev)
        for (d, w, attr, _q), v in zip(js, views):
            setattr(w, attr, _Pack16((_pack_stamp(d, w),) + getattr(w, attr).key[1:], v[0], v[1], inplace))


def _pack16_own_gen(weight):
    """generation of the weight's OWN in-place bf16 pack: moved by an on-the-spot rewrite of that one pack"""
    own = getattr(weight, "_mvd_pack16_own_gen", None)
    if own is None:
        own = weight._mvd_pack16_own_gen = [0]
    return own


def _pack16_guard(weight):
    """((generation holders), (generations now)) of the in-place bf16 packs `weight` takes part in, or None: the flat
    buffer's generation (the batched repack rewrites every pack of it) and the weight's own (_pack16_rewrite)."""
    flat = _flat_of(weight)
    holder = getattr(flat, "_mvd_pack16_gen", None) if flat is not None else None
    if holder is None:
        return None
    own = _pack16_own_gen(weight)
    return ((holder, own), (holder[0], own[0]))


def _check_pack16_generation(saved, what):
    if saved is not None and tuple(h[0] for h in saved[0]) != saved[1]:
        raise RuntimeError(f"{what}: the weights were updated (optimizer.step()) between the forward and the backward pass "
                           "of this graph; the bf16 packed copies saved for backward were rewritten in place")


def packs_stale(fp):
    """True when a cached pack of one of `fp`'s weights no longer carries the current stamp (a torch-visible write, e.g.
    load_state_dict, or invalidate_packs() since the last repack): a captured step, whose forward reads the persistent
    pack buffers, must not be replayed before repack_all(fp) has refreshed them."""
    for w, e in _live(_PACK_LIVE, "_mvd_pack", fp):
        if e.stamp != _pack_stamp(w.detach(), w):
            return True
    for attr, live in (("_mvd_pack16", _PACK16_LIVE), ("_mvd_pack16pad", _PACK16PAD_LIVE)):
        for w, e in _live(live, attr, fp):
            if e.key[0] != _pack_stamp(w.detach(), w):
                return True
    return False


def repack_all(fp=None):
    """Called by the fused optimizer after its update with its optim.FlatParams: new epoch of that flat buffer, every
    live cached weight that is a view of it re-packed in one launch.  Without `fp`: every live weight of the process
    (new global epoch)."""
    if fp is None:
        _PACK_EPOCH[0] += 1
    else:
        fp.flat._mvd_epoch[0] += 1
    _repack_all_bf16(fp)
    jobs = []
    for w, e in _live(_PACK_LIVE, "_mvd_pack", fp):
        d = w.detach()
        if d.is_cuda and d.dtype == torch.float32 and d.is_contiguous() and d.device == e.wf.device:
            jobs.append((d, e, w))
    if not jobs:
        return
    if any(e.uf is not None or e.ub is not None for _, e, _w in jobs) and query("mvd_wino_mode") != 2:
        return  # the batch entry only writes the F(2x2,3x3) layout; stale entries are packed per layer
    n = len(jobs)
    PA, IA = ctypes.c_void_p * n, ctypes.c_int * n
    ptr = lambda t: t.data_ptr() if t is not None else None
    w_ = PA(*[ptr(d) for d, _, _w in jobs])
    wf_ = PA(*[ptr(e.wf) for _, e, _w in jobs])
    wb_ = PA(*[ptr(e.wb) for _, e, _w in jobs])
    uf_ = PA(*[ptr(e.uf) for _, e, _w in jobs])
    ub_ = PA(*[ptr(e.ub) for _, e, _w in jobs])
    vf_ = PA(*[ptr(e.vf) for _, e, _w in jobs])
    vb_ = PA(*[ptr(e.vb) for _, e, _w in jobs])
    K_ = IA(*[e.K for _, e, _w in jobs])
    C_ = IA(*[e.C for _, e, _w in jobs])
    T_ = IA(*[e.T for _, e, _w in jobs])
    tr_ = IA(*[1 if e.transposed else 0 for _, e, _w in jobs])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    call("mvd_pack_weights_batch3", n, cast(w_), cast(wf_), cast(wb_), cast(uf_), cast(ub_), cast(vf_), cast(vb_), cast(K_),
         cast(C_), cast(T_), cast(tr_), _stream())
    for d, e, w in jobs:
        e.stamp = _pack_stamp(d, w)
        e.gen += 1


def pack_weight_bf16(weight, transposed):
    """fp32 master weight -> bf16 (wf16, wb16) in the MFMA 32x32x16 operand layout (mvd_pack_weight_bf16)."""
    w = weight.detach()
    if not w.is_contiguous():
        w = w.contiguous()
    if transposed:
        C, K = w.shape[:2]
    else:
        K, C = w.shape[:2]
    T = w[0, 0].numel()
    wf = torch.empty((T * C * K,), dtype=BF16, device=w.device)
    wb = torch.empty((T * C * K,), dtype=BF16, device=w.device)
    call("mvd_pack_weight_bf16", _p(w), _p(wf), _p(wb), K, C, T, 1 if transposed else 0, _stream())
    return wf, wb


def _packed_bf16(weight, transposed):
    """bf16 packs cached on the weight tensor under the same (epoch, version) stamp as the fp32 ones: inference packs
    once; in training the fused optimizer re-packs every registered weight in one launch after its update
    (repack_all -> mvd_pack_weights_bf16_batch_pad); a stale or missing entry is packed here, per layer -- into fresh
    tensors, or IN PLACE when the entry's tensors are views of a hipGraph trainer's persistent buffer (_pack16_rewrite)."""
    w = weight.detach()
    if not w.is_contiguous():
        return pack_weight_bf16(weight, transposed)
    e = getattr(weight, "_mvd_pack16", None)
    key = (_pack_stamp(w, weight), transposed, w.device)
    if e is None or e.key != key:
        if e is None:
            if len(_PACK16_LIVE) >= 4096:
                _PACK16_LIVE[:] = [r for r in _PACK16_LIVE if r() is not None]
            _PACK16_LIVE.append(weakref.ref(weight))
        if e is not None and e.inplace and e.key[1:] == key[1:]:
            e = _pack16_rewrite(weight, e, _pack16_shape(w, transposed=transposed))
        else:
            e = _Pack16(key, *pack_weight_bf16(weight, transposed))
        weight._mvd_pack16 = e
    return e.wf, e.wb


def _out_dim(i, k, s):
    return (i + 2 * ((k - 1) // 2) - k) // s + 1


# ======================================================================================================== gradient sharing
class _GradShare:
    """A tensor with two consumers gets two gradient contributions, which autograd adds with a torch elementwise kernel
    (a full read-read-write pass over the activation: 0.27 ms of the bf16 step, 0.48 ms of the fp32 step at configs[1]).
    share_grad() tags such a tensor; the consumer whose backward runs FIRST writes its contribution into a fresh buffer and
    publishes it here, the one that runs SECOND adds its contribution into that buffer inside its own kernel (epilogue
    read-modify-write) and returns None to autograd.  Autograd calls the producer's backward only after both consumers
    have run, so the buffer is complete when it is read.  A consumer without an accumulating kernel simply returns its own
    tensor (autograd adds, as before): any order and any mix stays correct."""
    __slots__ = ("buf",)

    def __init__(self):
        self.buf = None


def share_grad(t):
    if t.requires_grad:
        t._mvd_gshare = _GradShare()
    return t


def _share_of(t):
    return getattr(t, "_mvd_gshare", None)


def _publish(share, dx):
    """first contribution: remember the buffer (or drop a stale one when this consumer cannot accumulate)"""
    if share is not None:
        share.buf = dx
    return dx


def _joinable(share, shape, dtype):
    b = share.buf if share is not None else None
    return b if (b is not None and tuple(b.shape) == tuple(shape) and b.dtype == dtype and _is_cl3d(b)) else None


# ======================================================================================================== conv
class LaunchTimer:
    """bench.py: HIP events (on the stream the kernels run on) around the forward launches of ONE conv layer shape while
    the timed train steps run -- the in-step duration of the roofline kernel.  key = (bf16, N, C1, C2, K, D, H, W, kernel,
    stride); inactive unless `on`."""

    def __init__(self, key):
        self.key, self.pairs, self.on = tuple(key), [], False

    def mean_ms(self):
        return sum(a.elapsed_time(b) for a, b in self.pairs) / len(self.pairs) if self.pairs else None


LAUNCH_TIMER = None


BF16_CONV_STATS = [os.environ.get("MVD_BF16_CONV_STATS", "1") != "0"]
# fp32: InstanceNorm statistics from the epilogue of the direct conv kernels too (the first layer and the stride-2 layers; the
# Winograd layers always had it) -- MVD_DIRECT_CONV_STATS=0: the statistics pass over their outputs
DIRECT_CONV_STATS = [os.environ.get("MVD_DIRECT_CONV_STATS", "1") != "0"]


def conv3d_fwd_bf16(x1, C1, x2, C2, wf, bias, y, N, D, H, W, K, ks, stride, ws, in_scale=None, in_shift=None, slope=0.01):
    """mvd_conv3d_fwd_bf16, through the fused entry when the z-marching kernel takes the shape: the InstanceNorm
    statistics of the output then come out of the conv's epilogue (attached to `y` as `_mvd_tile_stats16`, picked up by
    InstanceNormLeakyReLUFn / NormActConv3dFn) and, with in_scale / in_shift, the input is normalised + activated in the
    loader (mvd_conv3d_fwd_bf16_fused)."""
    nt = query("mvd_conv3d_fwd_bf16_stats_tiles", N, D, H, W, C1, C2, K, i3(ks), i3(stride)) \
        if (BF16_CONV_STATS[0] or in_scale is not None) else 0
    if nt <= 0 and in_scale is None:
        call("mvd_conv3d_fwd_bf16", _p(x1), C1, _p(x2), C2, _p(wf), _p(bias), _p(y), N, D, H, W, K, i3(ks), i3(stride),
             _p(ws), ws.numel(), _stream())
        return
    stats = torch.empty((N, nt, K, 2), dtype=torch.float32, device=y.device) if (nt > 0 and BF16_CONV_STATS[0]) else None
    got = ctypes.c_int(0)
    call("mvd_conv3d_fwd_bf16_fused", _p(x1), C1, _p(x2), C2, _p(wf), _p(bias), _p(y), N, D, H, W, K, i3(ks), i3(stride),
         _p(in_scale), _p(in_shift), float(slope), _p(stats), ctypes.byref(got), _p(ws), ws.numel(), _stream())
    if stats is not None and got.value > 0:
        y._mvd_tile_stats16 = (stats, int(got.value))


class Conv3dFn(Function):
    """Conv3d(k in {1,3}, pad=(k-1)/2, stride in {1,2}) over the channel concat of x1 and (optional) x2.
    Replaces nn.Conv3d of ConvDropoutNormReLU and torch.cat((x, skip), 1) (UNetDecoder.py:107)."""

    @staticmethod
    def forward(ctx, x1, x2, weight, bias, stride):
        _require_cuda(x1, x2, weight, bias)
        ctx.share1, ctx.share2 = _share_of(x1), (_share_of(x2) if x2 is not None else None)
        x1 = to_ndhwc(x1)
        x2 = to_ndhwc(x2) if x2 is not None else None
        K, C = weight.shape[:2]
        ks = ks3(weight)
        N, C1, D, H, W = x1.shape
        C2 = x2.shape[1] if x2 is not None else 0
        if C1 + C2 != C:
            raise RuntimeError(f"conv3d: weight expects {C} input channels, got {C1}+{C2}")
        if weight.dim() == 4 and D != 1:
            raise RuntimeError("conv3d: a 2-D weight [K,C,kh,kw] needs [N,C,1,H,W] activations")
        if x2 is not None and tuple(x2.shape[2:]) != (D, H, W):
            raise RuntimeError("conv3d: the two concatenated inputs differ in spatial size")
        bf = _is_bf16(x1)
        if x2 is not None and _is_bf16(x2) != bf:
            raise RuntimeError("conv3d: the two concatenated inputs differ in dtype")
        od = [_out_dim(i, k, s) for i, k, s in zip((D, H, W), ks, stride)]
        y = empty_cl3d((N, K, *od), x1.device, x1.dtype)
        ws = _Workspace.get(query("mvd_conv_fwd_workspace_bytes", N, od[0] * od[1] * od[2], K), x1.device)
        ub = None
        tm = LAUNCH_TIMER
        timed = tm is not None and tm.on and tm.key == (bf, N, C1, C2, K, D, H, W, tuple(ks), tuple(stride))
        if timed:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record()
        if bf:
            wf, wb = _packed_bf16(weight, False)
            conv3d_fwd_bf16(x1, C1, x2, C2, wf, bias, y, N, D, H, W, K, ks, stride, ws)
        else:
            # fp32: one route query names the engine of the forward and of the input gradient (mvd_conv3d_route): 3x3x3
            # stride-1 layers run F(2x2x2,3x3x3) where it has enough work items and F(2x2,3x3) where that one has, the 9-tap
            # in-plane layers (1x3x3: a 2-D network's convs, anisotropic 3-D plans) F(2x2,3x3) per plane, the rest the direct
            # engines.  The packed weights and tables come from the per-weight cache (re-packed once per optimizer step, see
            # repack_all); uf / ub of a 9-tap weight are the in-plane engine's tables
            route = query("mvd_conv3d_route", N, D, H, W, C1, C2, K, i3(ks), i3(stride)) if len(ks) == 3 else 0
            kf, kb = route & 15, route >> 4
            two = (_lib.CONV_WINO2, _lib.CONV_WINO2P)
            pk = _packed(weight, False, kf in two, kb in two, kf == _lib.CONV_WINO3, kb == _lib.CONV_WINO3)
            wf, wb = pk.wf, pk.wb
            uf = pk.vf if kf == _lib.CONV_WINO3 else (pk.uf if kf in two else None)
            ub = pk.vb if kb == _lib.CONV_WINO3 else (pk.ub if kb in two else None)
            ctx.ub_kind = kb
            # statistics epilogue: the 3x3x3 Winograd kernels also emit the per-tile (sum, sum of squares) of their output, so
            # the InstanceNorm that follows (InstanceNormLeakyReLUFn picks them up from the tensor) skips its statistics pass;
            # the in-plane kernel has none (the norm behind it runs its pass).
            # The direct engines of the narrow-input and the stride-2 layers have the same epilogue; asked for only where
            # the norm behind the conv would otherwise run a statistics pass (a small volume takes its own, in one launch).
            # The trade: a chunked conv that is asked for statistics does not split its reduce channels over workgroups
            # (launch_fwd), which skinny problems -- few tiles, >= 32 reduce channels -- use to fill the chip.  In the
            # benchmark network no layer is both split and asked (the skinny stride-2 layers feed small norms); at other
            # patch sizes a chunked stride-2 layer with more than 1024 output voxels gives up its split for a statistics
            # pass of a few microseconds (MVD_DIRECT_CONV_STATS=0 keeps the split).
            ntiles = direct_tiles = 0
            if kf in (_lib.CONV_WINO2, _lib.CONV_WINO3):
                ntiles = query("mvd_conv_stats_tiles", od[0], od[1], od[2])
            elif kf == _lib.CONV_DIRECT and DIRECT_CONV_STATS[0] and len(ks) == 3 \
                    and not query("mvd_instnorm_single_launch", od[0] * od[1] * od[2], K):
                ntiles = direct_tiles = query("mvd_conv3d_fwd_stats_tiles", N, D, H, W, C1, C2, K, i3(ks), i3(stride))
            stats = torch.empty((N, ntiles, K, 2), dtype=torch.float32, device=x1.device) if ntiles > 0 else None
            done = ctypes.c_int(0)
            call("mvd_conv3d_fwd_routed", _p(x1), C1, _p(x2), C2, _p(wf), _p(uf), kf, _p(bias), _p(y), _p(stats), direct_tiles,
                 ctypes.byref(done), N, D, H, W, K, i3(ks), i3(stride), _p(ws), ws.numel(), _stream())
            if done.value:
                y._mvd_tile_stats = (stats, ntiles)
        if timed:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record()
            tm.pairs.append((ev0, ev1))
        ctx.bf = bf
        ctx.params = (weight, bias)
        ctx.pack = None if bf else (pk, pk.gen)
        ctx.pack16_gen = _pack16_guard(weight) if bf else None
        ctx.save_for_backward(x1, x2, wb, ub)
        ctx.geom = (N, C1, C2, D, H, W, K, ks, tuple(stride), tuple(od), bias is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x1, x2, wb, ub = ctx.saved_tensors
        _check_pack_generation(ctx.pack, "conv3d backward")  # (the bf16 packs are fresh tensors per stamp, or guarded:)
        _check_pack16_generation(ctx.pack16_gen, "conv3d backward")
        N, C1, C2, D, H, W, K, ks, stride, od, has_bias = ctx.geom
        dy = to_ndhwc(dy)
        dev = dy.device
        sfx = "_bf16" if ctx.bf else ""
        dx1 = dx2 = dw = db = None
        need1, need2 = ctx.needs_input_grad[0], (x2 is not None and ctx.needs_input_grad[1])
        joined = None
        if need1 and x2 is None and len(ks) == 3:
            # x1 has a second consumer whose backward already ran (a skip connection: the decoder conv read it through its
            # second pointer): add this conv's input gradient into that buffer inside the kernel
            joined = _joinable(ctx.share1, (N, C1, D, H, W), dy.dtype)
            if joined is not None and not query("mvd_conv3d_dgrad_acc_ok", int(ctx.bf), N, D, H, W, C1, K, i3(ks), i3(stride)):
                joined = None
        if joined is not None:
            if ctx.bf:
                ws = _Workspace.get(query("mvd_conv_fwd_workspace_bytes", N, D * H * W, C1), dev)
                call("mvd_conv3d_dgrad_bf16_acc", _p(dy), _p(wb), _p(joined), C1, N, D, H, W, K, i3(ks), i3(stride), _p(ws),
                     ws.numel(), _stream())
            else:
                call("mvd_conv3d_dgrad_acc", _p(dy), _p(wb), _p(joined), C1, N, D, H, W, K, i3(ks), i3(stride), _stream())
            ctx.share1.buf = None   # consumed
            need1 = False           # (None to autograd: the contribution already sits in the first consumer's tensor)
        elif need1 or need2:
            dx1 = empty_cl3d((N, C1, D, H, W), dev, dy.dtype)
            dx2 = empty_cl3d((N, C2, D, H, W), dev, dy.dtype) if x2 is not None else None
            ws = _Workspace.get(query("mvd_conv_fwd_workspace_bytes", N, D * H * W, C1 + C2), dev)
            if ctx.bf:
                call("mvd_conv3d_dgrad_bf16", _p(dy), _p(wb), _p(dx1), C1, _p(dx2), C2, N, D, H, W, K, i3(ks), i3(stride),
                     _p(ws), ws.numel(), _stream())
            else:
                call("mvd_conv3d_dgrad_routed", _p(dy), _p(wb), _p(ub), ctx.ub_kind, _p(dx1), C1, _p(dx2), C2, N, D, H, W, K,
                     i3(ks), i3(stride), _p(ws), ws.numel(), _stream())
            if need1:
                _publish(ctx.share1, dx1)
            if need2:
                _publish(ctx.share2, dx2)
        if ctx.needs_input_grad[2]:
            T = ks[0] * ks[1] * ks[2]
            weight, bias = ctx.params
            sink_w, sink_b = _take_grad(weight), (_take_grad(bias) if has_bias else None)
            dw = sink_w if sink_w is not None else torch.empty(tuple(weight.shape), dtype=torch.float32, device=dev)
            db = (sink_b if sink_b is not None else torch.empty((K,), dtype=torch.float32, device=dev)) if has_bias else None
            nb = query("mvd_conv3d_wgrad_workspace_bytes", C1 + C2, K, T, N, *od)
            ws = _Workspace.get(nb, dev)
            call("mvd_conv3d_wgrad" + sfx, _p(x1), C1, _p(x2), C2, _p(dy), _p(dw), _p(db), N, D, H, W, K, i3(ks), i3(stride),
                 _p(ws), ws.numel(), _stream())
            if sink_w is not None:
                dw = None
                _grad_done(weight)
            if sink_b is not None:
                db = None
                _grad_done(bias)
        return (dx1 if need1 else None), (dx2 if need2 else None), dw, db, None


def _padded_pack_bf16(weight, cpad):
    """bf16 packs of a [K][C][3][3][3] weight zero-padded to cpad reduce channels, cached under the usual stamp and
    registered like the plain bf16 packs: the fused optimizer rebuilds them in its batched repack, packs_stale() watches
    them, and in hipGraph mode they live in the persistent buffer.  The kernel pads while it packs (Csrc < C)."""
    w = weight.detach()

    def fresh(src):
        K, T = src.shape[0], src[0, 0].numel()
        wf = torch.empty((T * cpad * K,), dtype=BF16, device=src.device)
        wb = torch.empty((T * cpad * K,), dtype=BF16, device=src.device)
        _pack16_launch([(src, wf, wb) + _pack16_shape(src, cpad=cpad)], src.device)
        return wf, wb

    if not w.is_contiguous() or w.dtype != torch.float32:  # no cache for a strided view (the kernel reads plain fp32)
        return fresh(w.float().contiguous())
    e = getattr(weight, "_mvd_pack16pad", None)
    key = (_pack_stamp(w, weight), cpad, w.device)
    if e is None or e.key != key:
        if e is None:
            if len(_PACK16PAD_LIVE) >= 4096:
                _PACK16PAD_LIVE[:] = [r for r in _PACK16PAD_LIVE if r() is not None]
            _PACK16PAD_LIVE.append(weakref.ref(weight))
        if e is not None and e.inplace and e.key[1:] == key[1:]:
            e = _pack16_rewrite(weight, e, _pack16_shape(w, cpad=cpad))
        else:
            e = _Pack16(key, *fresh(w))
        weight._mvd_pack16pad = e
    return e.wf, e.wb


class NarrowInputConv3dBf16Fn(Function):
    """The network's input conv (4 modalities -> 32 channels, 3x3x3, stride 1) under bf16 mixed precision: the fp32 input
    is converted to bf16 NDHWC with the channels zero-padded to 32 (mvd_pad_channels_bf16) and the conv runs on the
    32-channel bf16 MFMA engines -- bf16 operands, fp32 accumulation, bf16 output, i.e. what the reference's autocast does
    to this layer (nnUNetTrainer.py:906) -- instead of the fp32 direct kernels (0.42 + 0.43 ms per step for a layer whose
    traffic is 0.34 GB).  The weight gradient of the zero channels is computed and dropped; the input needs no gradient."""
    CPAD = 32

    @staticmethod
    def forward(ctx, x, weight, bias):
        _require_cuda(x, weight, bias)
        if x.dtype != torch.float32:
            raise RuntimeError("narrow-input bf16 conv: the network input must be fp32")
        if ctx.needs_input_grad[0]:
            # (the backward of this layer has no input-gradient kernel; say so instead of returning None)
            raise RuntimeError("narrow-input bf16 conv: the gradient with respect to the network input is not on the path "
                               "(detach the input, or run the layer in fp32)")
        K, C = weight.shape[:2]
        if tuple(weight.shape[2:]) != (3, 3, 3) or K % 32 != 0 or C > 8 or x.shape[1] != C:
            raise RuntimeError("narrow-input bf16 conv: needs a 3x3x3 conv with <= 8 input and a multiple of 32 output channels")
        N, _, D, H, W = x.shape
        cl = _is_cl3d(x)
        if not cl and not x.is_contiguous():
            x = x.contiguous()
        cp = NarrowInputConv3dBf16Fn.CPAD
        xp = empty_cl3d((N, cp, D, H, W), x.device, BF16)
        call("mvd_pad_channels_bf16", _p(x), _p(xp), N, C, cp, D * H * W, 1 if cl else 0, _stream())
        wf, _wb = _padded_pack_bf16(weight, cp)
        y = empty_cl3d((N, K, D, H, W), x.device, BF16)
        ws = _Workspace.get(query("mvd_conv_fwd_workspace_bytes", N, D * H * W, K), x.device)
        conv3d_fwd_bf16(xp, cp, None, 0, wf, bias, y, N, D, H, W, K, (3, 3, 3), (1, 1, 1), ws)
        ctx.save_for_backward(xp)
        ctx.params = (weight, bias)
        ctx.geom = (N, C, D, H, W, K)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (xp,) = ctx.saved_tensors
        N, C, D, H, W, K = ctx.geom
        weight, bias = ctx.params
        dy = to_ndhwc(dy)
        dev = dy.device
        cp = NarrowInputConv3dBf16Fn.CPAD
        dw = db = None
        if ctx.needs_input_grad[1]:
            sink_w = _take_grad(weight)
            sink_b = _take_grad(bias) if bias is not None else None
            dwp = torch.empty((K, cp, 3, 3, 3), dtype=torch.float32, device=dev)
            db = (sink_b if sink_b is not None else torch.empty((K,), dtype=torch.float32, device=dev)) if bias is not None else None
            ws = _Workspace.get(query("mvd_conv3d_wgrad_workspace_bytes", cp, K, 27, N, D, H, W), dev)
            call("mvd_conv3d_wgrad_bf16", _p(xp), cp, None, 0, _p(dy), _p(dwp), _p(db), N, D, H, W, K, i3((3, 3, 3)),
                 i3((1, 1, 1)), _p(ws), ws.numel(), _stream())
            if sink_w is not None:
                sink_w.copy_(dwp[:, :C])
                _grad_done(weight)
            else:
                dw = dwp[:, :C].contiguous()
            if sink_b is not None:
                db = None
                _grad_done(bias)
        return None, dw, db


class ConvTranspose3dFn(Function):
    """ConvTranspose3d with kernel == stride (UNetDecoder.py:56-59)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        _require_cuda(x, weight, bias)
        ctx.share = _share_of(x)
        x = to_ndhwc(x)
        C, K = weight.shape[:2]
        if ks3(weight) != tuple(stride):
            raise RuntimeError("convT3d: only kernel_size == stride is on the hot path")
        N, Cx, D, H, W = x.shape
        if Cx != C:
            raise RuntimeError("convT3d: channel mismatch")
        bf = _is_bf16(x)
        if bf:
            wf, wb = _packed_bf16(weight, True)
        else:
            pk = _packed(weight, True)
            wf, wb = pk.wf, pk.wb
        y = empty_cl3d((N, K, D * stride[0], H * stride[1], W * stride[2]), x.device, x.dtype)
        ws = _Workspace.get(query("mvd_conv_fwd_workspace_bytes", N, D * H * W, K), x.device)
        ctx.bf = bf
        ctx.params = (weight, bias)
        ctx.pack = None if bf else (pk, pk.gen)
        ctx.pack16_gen = _pack16_guard(weight) if bf else None
        call("mvd_convT3d_fwd_bf16" if bf else "mvd_convT3d_fwd", _p(x), _p(wf), _p(bias), _p(y), N, D, H, W, C, K, i3(stride), _p(ws), ws.numel(),
             _stream())
        ctx.save_for_backward(x, wb)
        ctx.geom = (N, C, K, D, H, W, tuple(stride), bias is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, wb = ctx.saved_tensors
        _check_pack_generation(ctx.pack, "convT3d backward")
        _check_pack16_generation(ctx.pack16_gen, "convT3d backward")
        N, C, K, D, H, W, stride, has_bias = ctx.geom
        dy = to_ndhwc(dy)
        dev = dy.device
        dx = dw = db = None
        sfx = "_bf16" if ctx.bf else ""
        if ctx.needs_input_grad[0]:
            dx = empty_cl3d((N, C, D, H, W), dev, dy.dtype)
            ws = _Workspace.get(query("mvd_conv_fwd_workspace_bytes", N, D * H * W, C), dev)
            call("mvd_convT3d_dgrad" + sfx, _p(dy), _p(wb), _p(dx), N, D, H, W, C, K, i3(stride), _p(ws), ws.numel(),
                 _stream())
            _publish(ctx.share, dx)   # (no accumulating form of this kernel: always the first or a separate contribution)
        if ctx.needs_input_grad[1]:
            T = stride[0] * stride[1] * stride[2]
            weight, bias = ctx.params
            sink_w, sink_b = _take_grad(weight), (_take_grad(bias) if has_bias else None)
            dw = sink_w if sink_w is not None else torch.empty(tuple(weight.shape), dtype=torch.float32, device=dev)
            db = (sink_b if sink_b is not None else torch.empty((K,), dtype=torch.float32, device=dev)) if has_bias else None
            nb = query("mvd_convT3d_wgrad_workspace_bytes", C, K, T, N, D, H, W)
            ws = _Workspace.get(nb, dev)
            call("mvd_convT3d_wgrad" + sfx, _p(x), _p(dy), _p(dw), _p(db), N, D, H, W, C, K, i3(stride), _p(ws), ws.numel(),
                 _stream())
            if sink_w is not None:
                dw = None
                _grad_done(weight)
            if sink_b is not None:
                db = None
                _grad_done(bias)
        return dx, dw, db, None


# ======================================================================================================== norm
class InstanceNormLeakyReLUFn(Function):
    """InstanceNorm3d(eps, affine) + LeakyReLU(slope) fused (get_network_from_plans.py:41-44)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, slope, out_bf16=False):
        _require_cuda(x, gamma, beta)
        x = to_ndhwc(x)
        N, C = x.shape[:2]
        V = x[0, 0].numel()
        xb = _is_bf16(x)
        yb = bool(out_bf16) or xb  # a bf16 input never widens again inside the network
        y = empty_cl3d(x.shape, x.device, BF16 if yb else torch.float32)
        mean = torch.empty((N, C), dtype=torch.float32, device=x.device)
        rstd = torch.empty((N, C), dtype=torch.float32, device=x.device)
        nb = query("mvd_instnorm_workspace_bytes", N, V, C)
        ws = _Workspace.get(nb, x.device)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        pre = getattr(x, '_mvd_tile_stats', None)
        pre16 = getattr(x, '_mvd_tile_stats16', None) if xb else None
        if pre16 is not None and pre16[0].shape[0] == N and pre16[0].shape[2] == C and C % 4 == 0:
            # the bf16 conv's epilogue delivered the statistics: one finalize launch, then the apply pass in the
            # scale / shift form (the arithmetic of the fused loader prologue, mvd_conv3d_fwd_bf16_fused)
            scale, shift = torch.empty_like(mean), torch.empty_like(mean)
            call("mvd_instnorm_finalize_tiles", _p(pre16[0]), pre16[1], _p(g), _p(b), _p(mean), _p(rstd), _p(scale),
                 _p(shift), N, V, C, float(eps), _stream())
            call("mvd_instnorm_lrelu_apply_bf16", _p(x), _p(scale), _p(shift), _p(y), N, V, C, float(slope), _stream())
        elif yb:
            call("mvd_instnorm_lrelu_fwd_bf16", _p(x), int(xb), _p(g), _p(b), _p(y), _p(mean), _p(rstd), N, V, C,
                 float(eps), float(slope), _p(ws), ws.numel(), _stream())
        elif pre is not None and pre[0].shape[0] == N and pre[0].shape[2] == C:
            call("mvd_instnorm_lrelu_fwd_prestats", _p(x), _p(pre[0]), pre[1], _p(g), _p(b), _p(y), _p(mean), _p(rstd), N, V,
                 C, float(eps), float(slope), _p(ws), ws.numel(), _stream())
        else:
            call("mvd_instnorm_lrelu_fwd", _p(x), _p(g), _p(b), _p(y), _p(mean), _p(rstd), N, V, C, float(eps),
                 float(slope), _p(ws), ws.numel(), _stream())
        ctx.save_for_backward(x, g, b, mean, rstd)
        ctx.slope = float(slope)
        ctx.yb = yb
        ctx.params = (gamma, beta)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, g, b, mean, rstd = ctx.saved_tensors
        dy = to_ndhwc(dy)
        N, C = x.shape[:2]
        V = x[0, 0].numel()
        dx = empty_cl3d(x.shape, x.device, x.dtype)
        gamma, beta = ctx.params
        sink_g = _take_grad(gamma) if ctx.needs_input_grad[1] else None
        sink_b = _take_grad(beta) if ctx.needs_input_grad[2] else None
        dg = sink_g if sink_g is not None else torch.empty((C,), dtype=torch.float32, device=x.device)
        db = sink_b if sink_b is not None else torch.empty((C,), dtype=torch.float32, device=x.device)
        nb = query("mvd_instnorm_workspace_bytes", N, V, C)
        ws = _Workspace.get(nb, x.device)
        if ctx.yb:
            call("mvd_instnorm_lrelu_bwd_bf16", _p(x), int(_is_bf16(x)), _p(dy), _p(g), _p(b), _p(mean), _p(rstd), _p(dx),
                 _p(dg), _p(db), N, V, C, ctx.slope, _p(ws), ws.numel(), _stream())
        else:
            call("mvd_instnorm_lrelu_bwd", _p(x), _p(dy), _p(g), _p(b), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db), N, V,
                 C, ctx.slope, _p(ws), ws.numel(), _stream())
        if sink_g is not None:
            dg = None
            _grad_done(gamma)
        if sink_b is not None:
            db = None
            _grad_done(beta)
        return dx, dg, db, None, None, None


def _join_or_publish(share, shape, dev):
    """Gradient buffer of a tensor with several consumers, for a kernel that can accumulate: (buffer, accumulate, joined).
    joined: an earlier consumer's buffer exists, the kernel adds into it and the node returns None to autograd.  The buffer
    stays published (a later consumer may join too).  Otherwise a fresh buffer, published for the consumers still to run."""
    joined = _joinable(share, shape, torch.float32)
    if joined is not None:
        return joined, 1, True
    return _publish(share, empty_cl3d(shape, dev)), 0, False


class ResidualAddNormActFn(Function):
    """The tail of a residual block (BasicBlockD): y = LeakyReLU(IN(a) * gamma_a + beta_a + R), fp32 (mvd_resblock_fwd / _bwd).
    `a` is the raw output of conv2.  gamma_r is None: R = r (identity or pool-only skip); else r is the raw output of the
    skip branch's 1x1x1 projection and R = IN(r) * gamma_r + beta_r, normalised in the same pass.  Statistics a producing conv
    attached (`_mvd_tile_stats`) replace the pass over that tensor.  Backward: when r carries a shared gradient buffer
    (share_grad: the block input of the identity form feeds conv1 too) the kernel adds dr into it (`accumulate`)."""

    @staticmethod
    def forward(ctx, a, gamma_a, beta_a, r, gamma_r, beta_r, eps, slope):
        _require_cuda(a, gamma_a, beta_a, r, gamma_r, beta_r)
        proj = gamma_r is not None
        if proj and beta_r is None:
            raise RuntimeError("ResidualAddNormActFn: the projection form needs gamma_r and beta_r")
        if a.dtype != torch.float32 or r.dtype != torch.float32:
            raise NotImplementedError("ResidualEncoderUNet: the residual block tail is fp32 only (no bf16 mixed precision)")
        if tuple(a.shape) != tuple(r.shape) or a.dim() != 5:
            raise RuntimeError(f"residual block: conv branch {tuple(a.shape)} and skip branch {tuple(r.shape)} differ in shape")
        if any(p is not None and p.numel() != a.shape[1] for p in (gamma_a, beta_a, gamma_r, beta_r)):
            raise RuntimeError(f"residual block: the norm parameters must have {a.shape[1]} channels")
        ctx.share_r = _share_of(r)
        pre_a, pre_r = getattr(a, '_mvd_tile_stats', None), (getattr(r, '_mvd_tile_stats', None) if proj else None)
        a, r = to_ndhwc(a), to_ndhwc(r)
        N, C = a.shape[:2]
        V = a[0, 0].numel()
        dev = a.device
        y = empty_cl3d(a.shape, dev)
        ga, ba = gamma_a.detach().contiguous(), beta_a.detach().contiguous()
        gr, br = (gamma_r.detach().contiguous(), beta_r.detach().contiguous()) if proj else (None, None)
        mean_a = torch.empty((N, C), dtype=torch.float32, device=dev)
        rstd_a = torch.empty_like(mean_a)
        mean_r, rstd_r = (torch.empty_like(mean_a), torch.empty_like(mean_a)) if proj else (None, None)
        have = 0
        for bit, pre, m, s in ((1, pre_a, mean_a, rstd_a), (2, pre_r, mean_r, rstd_r)):
            if pre is not None and V > 1 and pre[0].shape[0] == N and pre[0].shape[2] == C:
                wsn = _Workspace.get(query("mvd_instnorm_workspace_bytes", N, V, C), dev)
                call("mvd_instnorm_stats_from_tiles", _p(pre[0]), pre[1], _p(m), _p(s), N, V, C, float(eps), _p(wsn), wsn.numel(),
                     _stream())
                have |= bit
        ws = _Workspace.get(query("mvd_resblock_workspace_bytes", N, V, C), dev)
        call("mvd_resblock_fwd", _p(a), _p(ga), _p(ba), _p(r), _p(gr), _p(br), _p(y), _p(mean_a), _p(rstd_a), _p(mean_r),
             _p(rstd_r), N, V, C, float(eps), float(slope), have, _p(ws), ws.numel(), _stream())
        ctx.proj = proj
        ctx.slope = float(slope)
        ctx.params = (gamma_a, beta_a, gamma_r, beta_r)
        if proj:
            ctx.save_for_backward(a, r, ga, ba, mean_a, rstd_a, gr, br, mean_r, rstd_r)
        else:
            ctx.save_for_backward(a, r, ga, ba, mean_a, rstd_a)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        if ctx.proj:
            a, r, ga, ba, mean_a, rstd_a, gr, br, mean_r, rstd_r = ctx.saved_tensors
        else:
            a, r, ga, ba, mean_a, rstd_a = ctx.saved_tensors
            gr = br = mean_r = rstd_r = None
        dy = to_ndhwc(dy)
        N, C = a.shape[:2]
        V = a[0, 0].numel()
        dev = a.device
        da = empty_cl3d(a.shape, dev)
        if ctx.needs_input_grad[3] and ctx.share_r is not None:
            dr, acc, joined = _join_or_publish(ctx.share_r, tuple(r.shape), dev)
        else:
            dr, acc, joined = empty_cl3d(r.shape, dev), 0, False
        params = ctx.params
        sinks = [(_take_grad(p) if p is not None else None) for p in params]
        outs = [(s if s is not None else torch.empty((C,), dtype=torch.float32, device=dev)) if p is not None else None
                for p, s in zip(params, sinks)]
        ws = _Workspace.get(query("mvd_resblock_workspace_bytes", N, V, C), dev)
        call("mvd_resblock_bwd", _p(a), _p(r), _p(dy), _p(ga), _p(ba), _p(mean_a), _p(rstd_a), _p(gr), _p(br), _p(mean_r),
             _p(rstd_r), _p(da), _p(dr), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), acc, N, V, C, ctx.slope, _p(ws),
             ws.numel(), _stream())
        for i, (p, s) in enumerate(zip(params, sinks)):
            if s is not None:
                outs[i] = None
                _grad_done(p)
        return da, outs[0], outs[1], (None if joined else dr), outs[2], outs[3], None, None


class AvgPool3dFn(Function):
    """AvgPool3d(stride, stride) of a strided residual block's skip branch on NDHWC fp32 (mvd_avgpool3d_fwd / _bwd); stride 1
    or 2 per axis, an odd extent on a strided axis is refused.  Backward joins a shared gradient buffer of x (`accumulate`)."""

    @staticmethod
    def forward(ctx, x, stride):
        _require_cuda(x)
        if x.dtype != torch.float32:
            raise NotImplementedError("ResidualEncoderUNet: the skip branch's average pool is fp32 only")
        stride = tuple(int(s) for s in stride)
        if x.dim() != 5 or len(stride) != 3:
            raise RuntimeError(f"avgpool3d: [N,C,D,H,W] and a 3-axis stride, got {tuple(x.shape)} and {stride}")
        ctx.share = _share_of(x)
        x = to_ndhwc(x)
        N, C, D, H, W = x.shape
        # (a stride other than 1 or 2 and an odd extent on a strided axis are refused by the library, before any launch)
        y = empty_cl3d((N, C, *[max(e // max(s, 1), 1) for e, s in zip((D, H, W), stride)]), x.device)
        call("mvd_avgpool3d_fwd", _p(x), _p(y), N, D, H, W, C, i3(stride), _stream())
        ctx.geom = (N, C, D, H, W, stride)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        N, C, D, H, W, stride = ctx.geom
        dy = to_ndhwc(dy)
        dx, acc, joined = _join_or_publish(ctx.share, (N, C, D, H, W), dy.device)
        call("mvd_avgpool3d_bwd", _p(dy), _p(dx), N, D, H, W, C, i3(stride), acc, _stream())
        return (None if joined else dx), None


class BatchNormLeakyReLUFn(Function):
    """BatchNorm3d(eps, affine, momentum, track_running_stats=True) + LeakyReLU(slope) fused (nnUNetTrainerBN.py:31-32).
    training: batch statistics over (N, D, H, W); the kernel updates running_mean / running_var / num_batches_tracked in
    place on the device (so a graph replay does too).  Otherwise one pass with the running statistics, which are only
    read.  Per-sample statistics a producing conv may have attached to x (_mvd_tile_stats / _mvd_tile_stats16) are not
    used: they are InstanceNorm's."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, slope, training,
                out_bf16=False):
        if gamma is None or beta is None:
            raise NotImplementedError("BatchNorm3d(affine=False) is not on the reference's path (nnUNetTrainerBN.py:32)")
        if running_mean is None or running_var is None or num_batches_tracked is None:
            raise NotImplementedError("BatchNorm3d(track_running_stats=False) is not built: the kernels keep running "
                                      "statistics")
        if momentum is None:
            raise NotImplementedError("BatchNorm3d(momentum=None), the cumulative moving average, is not built")
        N, C = x.shape[:2]
        V = x[0, 0].numel()
        if training and N * V == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        _require_cuda(x, gamma, beta, running_mean, running_var, num_batches_tracked)
        if not (running_mean.dtype == running_var.dtype == torch.float32 and num_batches_tracked.dtype == torch.int64 and
                running_mean.is_contiguous() and running_var.is_contiguous()):
            raise RuntimeError("batchnorm: running_mean / running_var must be contiguous fp32, num_batches_tracked int64")
        x = to_ndhwc(x)
        xb = _is_bf16(x)
        yb = bool(out_bf16) or xb  # a bf16 input never widens again inside the network
        y = empty_cl3d(x.shape, x.device, BF16 if yb else torch.float32)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        ctx.training = bool(training)
        if not training:
            call("mvd_batchnorm_lrelu_eval", _p(x), int(xb), _p(g), _p(b), _p(y), int(yb), _p(running_mean), _p(running_var),
                 N, V, C, float(eps), float(slope), _stream())
            return y
        mean = torch.empty((C,), dtype=torch.float32, device=x.device)
        rstd = torch.empty((C,), dtype=torch.float32, device=x.device)
        ws = _Workspace.get(query("mvd_batchnorm_workspace_bytes", N, V, C), x.device)
        call("mvd_batchnorm_lrelu_fwd", _p(x), int(xb), _p(g), _p(b), _p(y), int(yb), _p(mean), _p(rstd), _p(running_mean),
             _p(running_var), _p(num_batches_tracked), N, V, C, float(eps), float(momentum), float(slope), _p(ws), ws.numel(),
             _stream())
        ctx.save_for_backward(x, g, b, mean, rstd)
        ctx.slope = float(slope)
        ctx.yb = yb
        ctx.params = (gamma, beta)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        if not ctx.training:
            raise RuntimeError("batchnorm: backward through an eval-mode forward (running statistics) is not built; "
                               "call .train() before a step that differentiates")
        x, g, b, mean, rstd = ctx.saved_tensors
        dy = to_ndhwc(dy)
        N, C = x.shape[:2]
        V = x[0, 0].numel()
        dx = empty_cl3d(x.shape, x.device, x.dtype)
        gamma, beta = ctx.params
        sink_g = _take_grad(gamma) if ctx.needs_input_grad[1] else None
        sink_b = _take_grad(beta) if ctx.needs_input_grad[2] else None
        dg = sink_g if sink_g is not None else torch.empty((C,), dtype=torch.float32, device=x.device)
        db = sink_b if sink_b is not None else torch.empty((C,), dtype=torch.float32, device=x.device)
        ws = _Workspace.get(query("mvd_batchnorm_workspace_bytes", N, V, C), x.device)
        call("mvd_batchnorm_lrelu_bwd", _p(x), int(_is_bf16(x)), _p(dy), int(ctx.yb), _p(g), _p(b), _p(mean), _p(rstd),
             _p(dx), _p(dg), _p(db), N, V, C, ctx.slope, _p(ws), ws.numel(), _stream())
        if sink_g is not None:
            dg = None
            _grad_done(gamma)
        if sink_b is not None:
            db = None
            _grad_done(beta)
        return (dx, dg, db) + (None,) * 8


# NormActConv3dFn.backward: take the weight gradient through the loader prologue of k_wgrad16z (0: re-materialise the
# activated tensor with one apply pass first -- the A/B and cross-check switch)
WGRAD_PROLOGUE = os.environ.get("MVD_WGRAD_PROLOGUE", "1") != "0"


class NormActConv3dFn(Function):
    """The fused block boundary of the north_star (get_network_from_plans.py:41-44, bf16 mixed precision): InstanceNorm3d(affine)
    + LeakyReLU of block k folded into the LOADER of block k+1's Conv3d 3x3x3 (mvd_conv3d_fwd_bf16_fused: z-marching
    kernel, 32 -> 32 channels).  Input `y0` is the RAW bf16 output of block k's conv carrying the statistics its epilogue
    emitted (`_mvd_tile_stats16`); the activated tensor a0 = lrelu(IN(y0)) is never written in the forward pass.
    Backward: dgrad -> d a0; the InstanceNorm backward kernels on (y0, d a0) -> d y0, d gamma, d beta; the weight gradient
    needs a0 as an operand: mvd_conv3d_wgrad_bf16_fused re-computes it from y0 in ITS loader (k_wgrad16z, same arithmetic:
    bit-identical to the gradient over the materialised tensor), so a0 exists in neither pass.  Shapes that kernel does not
    serve fall back to one apply pass in front of the plain weight-gradient call."""

    @staticmethod
    def forward(ctx, y0, gamma, beta, eps, slope, weight, bias):
        _require_cuda(y0, gamma, beta, weight, bias)
        pre = getattr(y0, '_mvd_tile_stats16', None)
        if not (_is_bf16(y0) and _is_cl3d(y0)):
            raise RuntimeError("NormActConv3dFn: needs the raw bf16 NDHWC conv output")
        N, C, D, H, W = y0.shape
        K = weight.shape[0]
        V = D * H * W
        if tuple(weight.shape[1:]) != (C, 3, 3, 3):
            raise RuntimeError("NormActConv3dFn: 3x3x3 conv over the normalised tensor's channels")
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        mean = torch.empty((N, C), dtype=torch.float32, device=y0.device)
        rstd, scale, shift = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
        tm = LAUNCH_TIMER   # bench.py: the fused block (finalize + conv) inside the step
        timed = tm is not None and tm.on and tm.key == (True, N, C, 0, K, D, H, W, (3, 3, 3), (1, 1, 1))
        if timed:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record()
        if pre is not None and pre[0].shape[0] == N and pre[0].shape[2] == C:
            call("mvd_instnorm_finalize_tiles", _p(pre[0]), pre[1], _p(g), _p(b), _p(mean), _p(rstd), _p(scale), _p(shift), N,
                 V, C, float(eps), _stream())
        else:   # the producing conv ran on a kernel without the statistics epilogue: one pass over y0
            ws = _Workspace.get(query("mvd_instnorm_workspace_bytes", N, V, C), y0.device)
            call("mvd_instnorm_stats_bf16", _p(y0), 1, _p(g), _p(b), _p(mean), _p(rstd), _p(scale), _p(shift), N, V, C,
                 float(eps), _p(ws), ws.numel(), _stream())
        wf, wb = _packed_bf16(weight, False)
        y1 = empty_cl3d((N, K, D, H, W), y0.device, BF16)
        ws = _Workspace.get(query("mvd_conv_fwd_workspace_bytes", N, V, K), y0.device)
        conv3d_fwd_bf16(y0, C, None, 0, wf, bias, y1, N, D, H, W, K, (3, 3, 3), (1, 1, 1), ws, scale, shift, slope)
        if timed:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record()
            tm.pairs.append((ev0, ev1))
        ctx.save_for_backward(y0, g, b, mean, rstd, scale, shift, wb)
        ctx.params = (gamma, beta, weight, bias)
        ctx.slope = float(slope)
        ctx.pack16_gen = _pack16_guard(weight)
        return y1

    @staticmethod
    @once_differentiable
    def backward(ctx, dy1):
        y0, g, b, mean, rstd, scale, shift, wb = ctx.saved_tensors
        _check_pack16_generation(ctx.pack16_gen, "norm+act+conv3d backward")
        gamma, beta, weight, bias = ctx.params
        N, C, D, H, W = y0.shape
        K = weight.shape[0]
        V = D * H * W
        dev = y0.device
        dy1 = to_ndhwc(dy1)
        ks, st = i3((3, 3, 3)), i3((1, 1, 1))
        dy0 = dg = db_ = dw = db = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            da0 = empty_cl3d((N, C, D, H, W), dev, BF16)
            ws = _Workspace.get(query("mvd_conv_fwd_workspace_bytes", N, V, C), dev)
            call("mvd_conv3d_dgrad_bf16", _p(dy1), _p(wb), _p(da0), C, None, 0, N, D, H, W, K, ks, st, _p(ws), ws.numel(),
                 _stream())
            dy0 = empty_cl3d(y0.shape, dev, BF16)
            sink_g, sink_b = _take_grad(gamma), _take_grad(beta)
            dg = sink_g if sink_g is not None else torch.empty((C,), dtype=torch.float32, device=dev)
            db_ = sink_b if sink_b is not None else torch.empty((C,), dtype=torch.float32, device=dev)
            ws = _Workspace.get(query("mvd_instnorm_workspace_bytes", N, V, C), dev)
            call("mvd_instnorm_lrelu_bwd_bf16", _p(y0), 1, _p(da0), _p(g), _p(b), _p(mean), _p(rstd), _p(dy0), _p(dg), _p(db_),
                 N, V, C, ctx.slope, _p(ws), ws.numel(), _stream())
            if sink_g is not None:
                dg = None
                _grad_done(gamma)
            if sink_b is not None:
                db_ = None
                _grad_done(beta)
        if ctx.needs_input_grad[5]:
            has_bias = bias is not None
            sink_w, sink_b2 = _take_grad(weight), (_take_grad(bias) if has_bias else None)
            dw = sink_w if sink_w is not None else torch.empty((K, C, 3, 3, 3), dtype=torch.float32, device=dev)
            db = (sink_b2 if sink_b2 is not None else torch.empty((K,), dtype=torch.float32, device=dev)) if has_bias else None
            ws = _Workspace.get(query("mvd_conv3d_wgrad_workspace_bytes", C, K, 27, N, D, H, W), dev)
            if WGRAD_PROLOGUE and query("mvd_conv3d_wgrad_bf16_prologue_ok", N, D, H, W, C, 0, K, ks, st) > 0:
                # the weight-gradient kernel applies the same InstanceNorm + LeakyReLU to y0 in its loader: the activated
                # tensor is never materialised, in neither pass
                call("mvd_conv3d_wgrad_bf16_fused", _p(y0), C, _p(dy1), _p(dw), _p(db), N, D, H, W, K, ks, st, _p(scale),
                     _p(shift), ctx.slope, _p(ws), ws.numel(), _stream())
            else:
                a0 = empty_cl3d(y0.shape, dev, BF16)  # the activated tensor, only now (and only for the weight gradient)
                call("mvd_instnorm_lrelu_apply_bf16", _p(y0), _p(scale), _p(shift), _p(a0), N, V, C, ctx.slope, _stream())
                call("mvd_conv3d_wgrad_bf16", _p(a0), C, None, 0, _p(dy1), _p(dw), _p(db), N, D, H, W, K, ks, st, _p(ws),
                     ws.numel(), _stream())
            if sink_w is not None:
                dw = None
                _grad_done(weight)
            if sink_b2 is not None:
                db = None
                _grad_done(bias)
        return dy0, dg, db_, None, None, dw, db


def fused_norm_conv_ok(y0, weight, stride):
    """True when `y0` (raw bf16 conv output) can feed the next 3x3x3 conv through the fused loader
    prologue (mvd_conv3d_fwd_bf16_fused: the z-marching kernel takes the shape)."""
    if not (_is_bf16(y0) and y0.dim() == 5 and _is_cl3d(y0)):
        return False
    N, C, D, H, W = y0.shape
    K = weight.shape[0]
    if tuple(weight.shape[1:]) != (C, 3, 3, 3) or tuple(stride) != (1, 1, 1):
        return False
    return C % 4 == 0 and query("mvd_conv3d_fwd_bf16_prologue_ok", N, D, H, W, C, 0, K, i3((3, 3, 3)), i3((1, 1, 1))) > 0


# ======================================================================================================== seg head
class SegHeadFn(Function):
    """1x1x1 Conv3d C -> K producing planar logits [N,K,D,H,W] (UNetDecoder.py:70,110)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _require_cuda(x, weight, bias)
        ctx.share = _share_of(x)
        x = to_ndhwc(x)
        N, C = x.shape[:2]
        K = weight.shape[0]
        V = x[0, 0].numel()
        w = weight.detach().reshape(K, C).contiguous()
        logits = torch.empty((N, K, *x.shape[2:]), dtype=torch.float32, device=x.device)
        call("mvd_seghead_fwd_bf16" if _is_bf16(x) else "mvd_seghead_fwd", _p(x), _p(w), _p(bias), _p(logits), N, V, C, K,
             _stream())
        ctx.save_for_backward(x, w)
        ctx.wshape = tuple(weight.shape)
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, dl):
        x, w = ctx.saved_tensors
        N, C = x.shape[:2]
        K = w.shape[0]
        V = x[0, 0].numel()
        dl = dl.contiguous()
        dev = x.device
        # the other consumer of x (the next level's transposed conv) has already written its gradient: add ours into it
        joined = _joinable(ctx.share, x.shape, x.dtype) if ctx.needs_input_grad[0] else None
        dx = joined if joined is not None else (empty_cl3d(x.shape, dev, x.dtype) if ctx.needs_input_grad[0] else None)
        dw = torch.empty((K, C), dtype=torch.float32, device=dev)
        db = torch.empty((K,), dtype=torch.float32, device=dev)
        nb = query("mvd_seghead_bwd_workspace_bytes", N, V, C, K)
        ws = _Workspace.get(nb, dev)
        call("mvd_seghead_bwd_bf16" if _is_bf16(x) else "mvd_seghead_bwd", _p(x), _p(w), _p(dl), _p(dx), _p(dw), _p(db), N, V, C, K,
             1 if joined is not None else 0, _p(ws), ws.numel(), _stream())
        if ctx.share is not None:
            ctx.share.buf = None if joined is not None else dx   # consumed / first contribution
        return (None if joined is not None else dx), dw.view(ctx.wshape), db


# fp32 NormActSegHeadFn.backward: the InstanceNorm backward forms d a from the logit gradient in its own two passes
# (mvd_instnorm_lrelu_bwd_head) instead of reading a stored d a (MVD_NORM_BWD_FROM_DL=0: the two-call form; same bits)
NORM_BWD_FROM_DL = [os.environ.get("MVD_NORM_BWD_FROM_DL", "1") != "0"]


class NormActSegHeadFn(Function):
    """The LAST decoder block's InstanceNorm3d + LeakyReLU folded into the seg head that is its only consumer (UNetDecoder.py:110
    after get_network_from_plans.py:41-44): `y0` is the RAW output of the block's conv (with the statistics its epilogue
    emitted attached), the head kernels apply the normalisation + activation in their loaders (mvd_seghead_*_fused: bf16 in the
    scale / shift form of the bf16 apply pass, fp32 in the mean / rstd form of the fp32 one) -- the activated tensor of the
    top decoder stage is never written.  Backward: d a from the head's input-gradient kernel, the InstanceNorm backward on
    (y0, d a), dW / db over the re-computed a.  Bit-identical to the two separate nodes.  In fp32 d a is not stored either: the
    InstanceNorm backward forms it from the logit gradient and the head weight (NORM_BWD_FROM_DL), same bits again."""

    @staticmethod
    def forward(ctx, y0, gamma, beta, eps, slope, weight, bias):
        _require_cuda(y0, gamma, beta, weight, bias)
        bf = _is_bf16(y0)
        if not _is_cl3d(y0) or y0.dtype not in (BF16, torch.float32):
            raise RuntimeError("NormActSegHeadFn: needs the raw NDHWC conv output (bf16 or fp32)")
        N, C, D, H, W = y0.shape
        K = weight.shape[0]
        V = D * H * W
        dev = y0.device
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        mean = torch.empty((N, C), dtype=torch.float32, device=dev)
        rstd, scale, shift = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
        ws = _Workspace.get(query("mvd_instnorm_workspace_bytes", N, V, C), dev)
        pre16 = getattr(y0, '_mvd_tile_stats16', None) if bf else None
        pre = getattr(y0, '_mvd_tile_stats', None) if not bf else None
        if pre16 is not None and pre16[0].shape[0] == N and pre16[0].shape[2] == C:
            call("mvd_instnorm_finalize_tiles", _p(pre16[0]), pre16[1], _p(g), _p(b), _p(mean), _p(rstd), _p(scale), _p(shift), N,
                 V, C, float(eps), _stream())
        elif pre is not None and pre[0].shape[0] == N and pre[0].shape[2] == C:
            call("mvd_instnorm_stats_from_tiles", _p(pre[0]), pre[1], _p(mean), _p(rstd), N, V, C, float(eps), _p(ws), ws.numel(),
                 _stream())
        else:
            call("mvd_instnorm_stats_bf16", _p(y0), int(bf), _p(g), _p(b), _p(mean), _p(rstd), _p(scale), _p(shift), N, V, C,
                 float(eps), _p(ws), ws.numel(), _stream())
        w = weight.detach().reshape(K, C).contiguous()
        logits = torch.empty((N, K, D, H, W), dtype=torch.float32, device=dev)
        if bf:
            call("mvd_seghead_fwd_bf16_fused", _p(y0), _p(scale), _p(shift), float(slope), _p(w), _p(bias), _p(logits), N, V, C,
                 K, _stream())
        else:
            call("mvd_seghead_fwd_fused", _p(y0), _p(mean), _p(rstd), _p(g), _p(b), float(slope), _p(w), _p(bias), _p(logits), N,
                 V, C, K, _stream())
        ctx.save_for_backward(y0, g, b, mean, rstd, scale, shift, w)
        ctx.params = (gamma, beta)
        ctx.slope = float(slope)
        ctx.wshape = tuple(weight.shape)
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, dl):
        y0, g, b, mean, rstd, scale, shift, w = ctx.saved_tensors
        gamma, beta = ctx.params
        bf = _is_bf16(y0)
        N, C, D, H, W = y0.shape
        K = w.shape[0]
        V = D * H * W
        dev = y0.device
        dl = dl.contiguous()
        need_x = ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        from_dl = need_x and not bf and NORM_BWD_FROM_DL[0]
        da = empty_cl3d(y0.shape, dev, y0.dtype) if need_x and not from_dl else None
        dw = torch.empty((K, C), dtype=torch.float32, device=dev)
        db = torch.empty((K,), dtype=torch.float32, device=dev)
        ws = _Workspace.get(query("mvd_seghead_bwd_workspace_bytes", N, V, C, K), dev)
        if bf:
            call("mvd_seghead_bwd_bf16_fused", _p(y0), _p(scale), _p(shift), ctx.slope, _p(w), _p(dl), _p(da), _p(dw), _p(db), N,
                 V, C, K, 0, _p(ws), ws.numel(), _stream())
        else:
            call("mvd_seghead_bwd_fused", _p(y0), _p(mean), _p(rstd), _p(g), _p(b), ctx.slope, _p(w), _p(dl), _p(da), _p(dw),
                 _p(db), N, V, C, K, 0, _p(ws), ws.numel(), _stream())
        dy0 = dg = db_ = None
        if need_x:
            dy0 = empty_cl3d(y0.shape, dev, y0.dtype)
            sink_g, sink_b = _take_grad(gamma), _take_grad(beta)
            dg = sink_g if sink_g is not None else torch.empty((C,), dtype=torch.float32, device=dev)
            db_ = sink_b if sink_b is not None else torch.empty((C,), dtype=torch.float32, device=dev)
            ws = _Workspace.get(query("mvd_instnorm_workspace_bytes", N, V, C), dev)
            if from_dl:
                call("mvd_instnorm_lrelu_bwd_head", _p(y0), _p(dl), _p(w), K, _p(g), _p(b), _p(mean), _p(rstd), _p(dy0), _p(dg),
                     _p(db_), N, V, C, ctx.slope, _p(ws), ws.numel(), _stream())
            elif bf:
                call("mvd_instnorm_lrelu_bwd_bf16", _p(y0), 1, _p(da), _p(g), _p(b), _p(mean), _p(rstd), _p(dy0), _p(dg),
                     _p(db_), N, V, C, ctx.slope, _p(ws), ws.numel(), _stream())
            else:
                call("mvd_instnorm_lrelu_bwd", _p(y0), _p(da), _p(g), _p(b), _p(mean), _p(rstd), _p(dy0), _p(dg), _p(db_), N, V,
                     C, ctx.slope, _p(ws), ws.numel(), _stream())
            if sink_g is not None:
                dg = None
                _grad_done(gamma)
            if sink_b is not None:
                db_ = None
                _grad_done(beta)
        return dy0, dg, db_, None, None, dw.view(ctx.wshape), db


def fused_norm_seghead_ok(y0, weight):
    """True when the seg head can read the raw (bf16 or fp32) conv output `y0` through its fused loaders."""
    if not (y0.dtype in (BF16, torch.float32) and y0.dim() == 5 and _is_cl3d(y0) and y0.is_cuda):
        return False
    N, C = y0.shape[:2]
    return weight.shape[1] == C and query("mvd_seghead_bf16_fused_ok", N, y0[0, 0].numel(), C, weight.shape[0]) > 0


class CastFn(Function):
    """Precision boundary: bf16 activation -> fp32 (and the fp32 gradient back to bf16), layout preserved.  Used where
    a bf16 feature map feeds an fp32 loss kernel (the distillation features)."""

    @staticmethod
    def forward(ctx, x):
        _require_cuda(x)
        if not _is_bf16(x):
            raise RuntimeError("CastFn widens bf16 tensors")
        x = to_ndhwc(x)
        y = torch.empty_like(x, dtype=torch.float32)  # preserves the NDHWC strides
        call("mvd_cast_bf16_to_f32", _p(x), _p(y), x.numel(), _stream())
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = to_ndhwc(dy)
        dx = torch.empty_like(dy, dtype=BF16)
        call("mvd_cast_f32_to_bf16", _p(dy), _p(dx), dy.numel(), _stream())
        return dx


def widen(x):
    """fp32 view of an activation for the fp32 loss kernels (identity in the fp32 mode)."""
    return CastFn.apply(x) if _is_bf16(x) else x


# ======================================================================================================== losses
def _flat_target(t, N, V):
    """float label map [N,1,...] or [N,...] -> contiguous [N,V]."""
    t = t.reshape(N, -1)
    if t.shape[1] != V:
        raise RuntimeError(f"target has {t.shape[1]} voxels per sample, logits have {V}")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


class DeepSupervisedDCCEFn(Function):
    """sum_i w_i * (w_ce*CE(x_i,t_i) + w_dice*(-softDice(softmax(x_i),t_i))) in one autograd node
    (DeepSupervisionWrapper o DC_and_CE_loss, nnUNetTrainer.py:359-374).  Levels with w_i == 0 contribute exact-zero
    gradients (upstream 2.1.1 evaluates them; see oracle/loss_oracle.py).  `gather` (optional) maps the per-sample
    stats [N,3K+1] to the all-gathered stats for DDP batch-dice (collective C2); it returns (stats_all, my_offset,
    grad_multiplier)."""

    @staticmethod
    def forward(ctx, weights, cfg, gather, targets, *logits):
        batch_dice, do_bg, smooth, w_ce, w_dice = cfg
        dev = logits[0].device
        total = torch.zeros((1,), dtype=torch.float32, device=dev)
        saved = []
        ctx.levels = []
        for i, (x, t) in enumerate(zip(logits, targets)):
            if weights[i] == 0:
                ctx.levels.append(None)
                continue
            _require_cuda(x, t)
            x = x.contiguous()
            N, K = x.shape[:2]
            V = x[0, 0].numel()
            t = _flat_target(t, N, V)
            stats = torch.empty((N, 3 * K + 1), dtype=torch.float32, device=dev)
            nb = query("mvd_dcce_workspace_bytes", N, V, K)
            ws = _Workspace.get(nb, dev)
            call("mvd_dcce_fwd", _p(x), _p(t), _p(stats), N, V, K, _p(ws), ws.numel(), _stream())
            dstats, off, mult = (stats, 0, 1.0)
            if gather is not None and batch_dice:
                dstats, off, mult = gather(stats)
            Nd = dstats.shape[0]
            loss = torch.empty((3,), dtype=torch.float32, device=dev)
            coef = torch.empty((Nd, K, 2), dtype=torch.float32, device=dev)
            call("mvd_dcce_finalize", _p(stats), N, _p(dstats), Nd, _p(loss), _p(coef), V, K, int(batch_dice), int(do_bg),
                 float(smooth), float(w_ce), float(w_dice), _stream())
            call("mvd_axpy", _p(total), _p(loss), float(weights[i]), 1, _stream())
            saved += [x, t, coef[off:off + N].contiguous() if (off or Nd != N) else coef]
            ctx.levels.append((N, K, V, float(weights[i]) , float(mult)))
        ctx.save_for_backward(*saved)
        ctx.w_ce = float(w_ce)
        ctx.shapes = [tuple(x.shape) for x in logits]
        return total.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        saved = ctx.saved_tensors
        g = g.contiguous()
        grads = []
        j = 0
        for lvl, shp in zip(ctx.levels, ctx.shapes):
            if lvl is None:
                grads.append(torch.zeros(shp, dtype=torch.float32, device=g.device))
                continue
            N, K, V, w, mult = lvl
            x, t, coef = saved[j:j + 3]
            j += 3
            if mult != 1.0:
                coef = coef * mult  # ddp batch-dice: AllGatherGrad.backward sums the (identical) grads of all ranks
            dl = torch.empty(shp, dtype=torch.float32, device=g.device)
            call("mvd_dcce_bwd", _p(x), _p(t), _p(coef), _p(g), w, _p(dl), N, V, K, ctx.w_ce, _stream())
            grads.append(dl)
        return (None, None, None, None, *grads)


def argmax_counts(logits, target):
    """validation_step online evaluation (nnUNetTrainer.py:973-990): returns int64 [K,3] = (tp, fp, fn) per class."""
    _require_cuda(logits, target)
    x = logits.contiguous()
    N, K = x.shape[:2]
    V = x[0, 0].numel()
    t = _flat_target(target, N, V)
    counts = torch.empty((K, 3), dtype=torch.int64, device=x.device)
    call("mvd_argmax_counts", _p(x), _p(t), _p(counts), N, V, K, _stream())
    return counts


# ------------------------------------------------------------------------------- regions / ignore label
REGION_KMAX = 8  # heads of the fused loss kernels (KMAX in csrc/loss.hip, RKMAX in csrc/loss_region.hip)
IGNORE_BIT = 1 << 31


def region_label_table(regions, ignore_label=None):
    """label -> bitmask table of the region kernels, uint32 [256]: bit r is set when the label belongs to regions[r] (an
    int or a tuple / list of ints), bit 31 when it is the ignore label (region_based_training.py:23-38 as a lookup)."""
    if len(regions) > 31:
        raise NotImplementedError(f"{len(regions)} regions: the label table holds 31")
    lut = np.zeros(256, dtype=np.uint32)
    for r, reg in enumerate(regions):
        for l in (reg if isinstance(reg, (list, tuple)) else (reg,)):
            l = int(l)
            if not 0 <= l <= 255:
                raise NotImplementedError(f"label {l} outside 0..255")
            lut[l] |= np.uint32(1 << r)
    if ignore_label is not None:
        if not 0 <= int(ignore_label) <= 255:
            raise NotImplementedError(f"ignore label {ignore_label} outside 0..255")
        lut[int(ignore_label)] |= np.uint32(IGNORE_BIT)
    return lut


def _lut_p(lut):
    return None if lut is None else lut.ctypes.data_as(ctypes.c_void_p)


def _region_target(t, N, R, V, form):
    """form 0: float label map -> [N,V]; 1 / 2: planes [N,R(+1),...] -> [N,R(+1),V]."""
    if form == 0:
        return _flat_target(t, N, V)
    TP = R + (1 if form == 2 else 0)
    if t.dim() < 3 or t.shape[0] != N or t.shape[1] != TP or t[0, 0].numel() != V:
        raise RuntimeError(f"region target must be [{N}, {TP}, ...] planes with {V} voxels each (the ignore plane last), "
                           f"got {tuple(t.shape)}")
    t = t.reshape(N, TP, V)
    return (t if t.dtype == torch.float32 else t.float()).contiguous()


def _check_heads(K):
    if K > REGION_KMAX:
        raise NotImplementedError(f"{K} segmentation heads: the fused loss kernels hold at most {REGION_KMAX}")


class DeepSupervisedMaskedFn(Function):
    """DeepSupervisedDCCEFn's sibling for the two label modes it does not cover, again one autograd node over all levels:
    cfg = ('bce', batch_dice, do_bg, smooth, w_ce, w_dice, (target_form, lut, use_ignore_label)): DC_and_BCE_loss over
    sigmoid heads (mvd_dcbce_*);  ('ce', ..., ignore_label): DC_and_CE_loss(ignore_label=) (mvd_dcce_masked_*).
    Stats are [N, 3K+2]; `gather` as in DeepSupervisedDCCEFn (parallel.gather_dice_stats is width-agnostic)."""

    @staticmethod
    def forward(ctx, weights, cfg, gather, targets, *logits):
        mode, batch_dice, do_bg, smooth, w_ce, w_dice, extra = cfg
        dev = logits[0].device
        total = torch.zeros((1,), dtype=torch.float32, device=dev)
        saved = []
        ctx.levels = []
        for i, (x, t) in enumerate(zip(logits, targets)):
            if weights[i] == 0:
                ctx.levels.append(None)
                continue
            _require_cuda(x, t)
            x = x.contiguous()
            N, K = x.shape[:2]
            _check_heads(K)
            V = x[0, 0].numel()
            stats = torch.empty((N, 3 * K + 2), dtype=torch.float32, device=dev)
            if mode == 'bce':
                form, lut, use_ignore = extra
                t = _region_target(t, N, K, V, form)
                ws = _Workspace.get(query("mvd_dcbce_workspace_bytes", N, V, K), dev)
                call("mvd_dcbce_fwd", _p(x), _p(t), form, _lut_p(lut), _p(stats), N, V, K, _p(ws), ws.numel(), _stream())
            else:
                t = _flat_target(t, N, V)
                ws = _Workspace.get(query("mvd_dcce_masked_workspace_bytes", N, V, K), dev)
                call("mvd_dcce_masked_fwd", _p(x), _p(t), _p(stats), N, V, K, int(extra), _p(ws), ws.numel(), _stream())
            dstats, off, mult = (stats, 0, 1.0)
            if gather is not None and batch_dice:
                dstats, off, mult = gather(stats)
            Nd = dstats.shape[0]
            loss = torch.empty((4,), dtype=torch.float32, device=dev)
            coef = torch.empty((Nd, K, 2), dtype=torch.float32, device=dev)
            if mode == 'bce':
                call("mvd_dcbce_finalize", _p(stats), N, _p(dstats), Nd, _p(loss), _p(coef), V, K, int(batch_dice),
                     int(do_bg), int(use_ignore), float(smooth), float(w_ce), float(w_dice), _stream())
            else:
                call("mvd_dcce_masked_finalize", _p(stats), N, _p(dstats), Nd, _p(loss), _p(coef), V, K, int(batch_dice),
                     int(do_bg), float(smooth), float(w_ce), float(w_dice), _stream())
            call("mvd_axpy", _p(total), _p(loss), float(weights[i]), 1, _stream())
            saved += [x, t, coef[off:off + N].contiguous() if (off or Nd != N) else coef, loss]
            ctx.levels.append((N, K, V, float(weights[i]), float(mult)))
        ctx.save_for_backward(*saved)
        ctx.mode, ctx.extra, ctx.w_ce = mode, extra, float(w_ce)
        ctx.shapes = [tuple(x.shape) for x in logits]
        return total.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        saved = ctx.saved_tensors
        g = g.contiguous()
        grads = []
        j = 0
        for lvl, shp in zip(ctx.levels, ctx.shapes):
            if lvl is None:
                grads.append(torch.zeros(shp, dtype=torch.float32, device=g.device))
                continue
            N, K, V, w, mult = lvl
            x, t, coef, loss = saved[j:j + 4]
            j += 4
            if mult != 1.0:
                coef = coef * mult
            dl = torch.empty(shp, dtype=torch.float32, device=g.device)
            if ctx.mode == 'bce':
                form, lut, _ = ctx.extra
                call("mvd_dcbce_bwd", _p(x), _p(t), form, _lut_p(lut), _p(coef), _p(loss), _p(g), w, _p(dl), N, V, K,
                     ctx.w_ce, _stream())
            else:
                call("mvd_dcce_masked_bwd", _p(x), _p(t), _p(coef), _p(loss), _p(g), w, _p(dl), N, V, K, ctx.w_ce,
                     int(ctx.extra), _stream())
            grads.append(dl)
        return (None, None, None, None, *grads)


def topk_count(n, k_percent):
    """robust_ce_loss.py:30-31: int(num_voxels * k / 100) with num_voxels an np.int64."""
    return int(np.int64(n) * k_percent / 100)


class DeepSupervisedTopKFn(Function):
    """sum_i w_i * (w_ce * TopK(x_i, t_i) [+ w_dice * (-softDice)]) in one autograd node: TopKLoss
    (robust_ce_loss.py:19-32) and upstream 2.1.1's DC_and_topk_loss.  cfg = (k_percent, label_smoothing, ignore_index,
    dice) with dice None or (batch_dice, do_bg, smooth, w_ce, w_dice, ignore_label): the Dice statistics and coefficients
    come from mvd_dcce_fwd / mvd_dcce_finalize (their _masked_ forms with an ignore label) run with w_ce = 0, the
    gradient is written once by mvd_topk_bwd.  `gather` as in DeepSupervisedDCCEFn, for the Dice half only: the top-k is
    local to the rank.  Levels with w_i == 0 contribute exact-zero gradients.  Per level the forward saves the per-voxel
    CE (4 B per voxel) and the selection state {t_bits, cnt_gt, cnt_eq}: the backward reads them, it recomputes neither."""

    @staticmethod
    def forward(ctx, weights, cfg, gather, targets, *logits):
        k_percent, eps, ignore_index, dice = cfg
        dev = logits[0].device
        total = torch.zeros((1,), dtype=torch.float32, device=dev)
        saved = []
        ctx.levels = []
        for i, (x, t) in enumerate(zip(logits, targets)):
            if weights[i] == 0:
                ctx.levels.append(None)
                continue
            _require_cuda(x, t)
            x = x.contiguous()
            N, K = x.shape[:2]
            _check_heads(K)
            V = x[0, 0].numel()
            k = topk_count(N * V, k_percent)
            if k < 1:
                raise ValueError(f"top-k loss: k = int({N * V} voxels * {k_percent} / 100) = 0; the reference's mean over an "
                                 f"empty selection is NaN.  A level needs at least {int(np.ceil(100 / k_percent))} voxels")
            t = _flat_target(t, N, V)
            coef, w_ce, mult, dloss = None, 1.0, 1.0, None
            if dice is not None:
                batch_dice, do_bg, smooth, w_ce, w_dice, ignore_label = dice
                masked = ignore_label is not None
                stats = torch.empty((N, 3 * K + (2 if masked else 1)), dtype=torch.float32, device=dev)
                if masked:
                    ws = _Workspace.get(query("mvd_dcce_masked_workspace_bytes", N, V, K), dev)
                    call("mvd_dcce_masked_fwd", _p(x), _p(t), _p(stats), N, V, K, int(ignore_label), _p(ws), ws.numel(),
                         _stream())
                else:
                    ws = _Workspace.get(query("mvd_dcce_workspace_bytes", N, V, K), dev)
                    call("mvd_dcce_fwd", _p(x), _p(t), _p(stats), N, V, K, _p(ws), ws.numel(), _stream())
                dstats, off = stats, 0
                if gather is not None and batch_dice:
                    dstats, off, mult = gather(stats)
                Nd = dstats.shape[0]
                dloss = torch.empty((4,), dtype=torch.float32, device=dev)
                coef = torch.empty((Nd, K, 2), dtype=torch.float32, device=dev)
                call("mvd_dcce_masked_finalize" if masked else "mvd_dcce_finalize", _p(stats), N, _p(dstats), Nd, _p(dloss),
                     _p(coef), V, K, int(batch_dice), int(do_bg), float(smooth), 0.0, float(w_dice), _stream())
                if off or Nd != N:
                    coef = coef[off:off + N].contiguous()
                if mult != 1.0:
                    coef = coef * mult   # ddp batch-dice: AllGatherGrad.backward sums the (identical) grads of all ranks
            ce = torch.empty((N, V), dtype=torch.float32, device=dev)
            state = torch.empty((4,), dtype=torch.int32, device=dev)
            loss = torch.empty((2,), dtype=torch.float32, device=dev)
            call("mvd_topk_ce_fwd", _p(x), _p(t), _p(ce), N, V, K, int(ignore_index), float(eps), _stream())
            ws = _Workspace.get(query("mvd_topk_workspace_bytes", N, V), dev)
            call("mvd_topk_select", _p(ce), N * V, k, _p(state), _p(ws), ws.numel(), _stream())
            call("mvd_topk_finalize", _p(ce), N * V, k, _p(state), float(w_ce), _p(dloss), _p(loss), _p(ws), ws.numel(),
                 _stream())
            call("mvd_axpy", _p(total), _p(loss), float(weights[i]), 1, _stream())
            saved += [x, t, ce, state] + ([coef] if coef is not None else [])
            ctx.levels.append((N, K, V, k, float(weights[i]), float(w_ce), coef is not None))
        ctx.save_for_backward(*saved)
        ctx.eps, ctx.ignore_index = float(eps), int(ignore_index)
        ctx.shapes = [tuple(x.shape) for x in logits]
        return total.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        saved = ctx.saved_tensors
        g = g.contiguous()
        grads = []
        j = 0
        for lvl, shp in zip(ctx.levels, ctx.shapes):
            if lvl is None:
                grads.append(torch.zeros(shp, dtype=torch.float32, device=g.device))
                continue
            N, K, V, k, w, w_ce, has_dice = lvl
            x, t, ce, state = saved[j:j + 4]
            coef = saved[j + 4] if has_dice else None
            j += 5 if has_dice else 4
            dl = torch.empty(shp, dtype=torch.float32, device=g.device)
            call("mvd_topk_bwd", _p(x), _p(t), _p(ce), _p(state), _p(coef), _p(g), w, _p(dl), N, V, K, k, w_ce,
                 ctx.ignore_index, ctx.eps, _stream())
            grads.append(dl)
        return (None, None, None, None, *grads)


def topk_ce(logits, target, ignore_index=-100, label_smoothing=0.0):
    """The per-voxel CE buffer [N,V] the top-k selection runs on (cross_entropy(reduction='none'), ignored voxels +0.0)."""
    _require_cuda(logits, target)
    x = logits.contiguous()
    N, K = x.shape[:2]
    _check_heads(K)
    V = x[0, 0].numel()
    ce = torch.empty((N, V), dtype=torch.float32, device=x.device)
    call("mvd_topk_ce_fwd", _p(x), _p(_flat_target(target, N, V)), _p(ce), N, V, K, int(ignore_index), float(label_smoothing),
         _stream())
    return ce


def topk_select(ce, k):
    """The selection alone on a device buffer of non-negative fp32 values: int64 [3] = (t_bits, cnt_gt, cnt_eq) of its
    k-th largest (what DeepSupervisedTopKFn runs per level; the tests check it against a host sort of the same buffer)."""
    _require_cuda(ce)
    ce = ce.contiguous().reshape(-1)
    state = torch.empty((4,), dtype=torch.int32, device=ce.device)
    ws = _Workspace.get(query("mvd_topk_workspace_bytes", 1, ce.numel()), ce.device)
    call("mvd_topk_select", _p(ce), ce.numel(), int(k), _p(state), _p(ws), ws.numel(), _stream())
    return state[:3].to(torch.int64) & 0xffffffff


def argmax_counts_masked(logits, target, ignore_label):
    """validation_step with an ignore label and softmax heads (nnUNetTrainer.py:980-990): argmax_counts over the voxels
    whose target is not ignore_label.  int64 [K,3]."""
    _require_cuda(logits, target)
    x = logits.contiguous()
    N, K = x.shape[:2]
    _check_heads(K)
    V = x[0, 0].numel()
    t = _flat_target(target, N, V)
    counts = torch.empty((K, 3), dtype=torch.int64, device=x.device)
    call("mvd_argmax_counts_masked", _p(x), _p(t), _p(counts), N, V, K, int(ignore_label), _stream())
    return counts


def sigmoid_counts(logits, target, regions=None, ignore_label=None, has_ignore_plane=False):
    """validation_step for region heads (:969-990): head r predicts a voxel where its logit is > 0 (sigmoid > 0.5); int64
    [R,3] = (tp, fp, fn) per region over the voxels that are not ignored.  `regions` given: target is the float label map
    and ignore_label its ignore label; absent: target holds the [N,R(+1),...] planes (has_ignore_plane: the last one)."""
    _require_cuda(logits, target)
    x = logits.contiguous()
    N, R = x.shape[:2]
    _check_heads(R)
    V = x[0, 0].numel()
    if regions is not None:
        if len(regions) != R:
            raise RuntimeError(f"{len(regions)} regions for {R} heads")
        form, lut = 0, region_label_table(regions, ignore_label)
    else:
        form, lut = (2 if has_ignore_plane else 1), None
    t = _region_target(target, N, R, V, form)
    counts = torch.empty((R, 3), dtype=torch.int64, device=x.device)
    call("mvd_sigmoid_counts", _p(x), _p(t), form, _lut_p(lut), _p(counts), N, V, R, _stream())
    return counts


def convert_seg_to_regions(seg, regions, ignore_label=None):
    """ConvertSegmentationToRegionsTransform (region_based_training.py:23-38) on the device: label map [N,1,...] or
    [N,...] -> float32 planes [N, R(+1), ...], the ignore label's plane last (nnUNetTrainer.py:759-763)."""
    _require_cuda(seg)
    if seg.dim() >= 3 and seg.shape[1] == 1:
        spatial = tuple(seg.shape[2:])
    else:
        spatial = tuple(seg.shape[1:])
    N = seg.shape[0]
    V = int(np.prod(spatial))
    t = _flat_target(seg, N, V)
    R = len(regions)
    TP = R + (1 if ignore_label is not None else 0)
    out = torch.empty((N, TP, *spatial), dtype=torch.float32, device=seg.device)
    call("mvd_seg_to_regions", _p(t), _lut_p(region_label_table(regions, ignore_label)), _p(out), N, V, R,
         int(ignore_label is not None), _stream())
    return out


def _kl_strides(t):
    """(N, C, V, sn, sc, sv) of a [N,C,*spatial] tensor whose spatial block is dense in either planar or NDHWC order."""
    N, C = t.shape[:2]
    V = t[0, 0].numel()
    if t.is_contiguous():
        return N, C, V, C * V, V, 1
    if _is_cl3d(t):
        return N, C, V, C * V, 1, C
    # channel slice of a planar tensor ([N,1,...] view with batch stride K*V)
    st = t.stride()
    sp = t[0, 0]
    if sp.is_contiguous():
        return N, C, V, st[0], st[1], 1
    raise RuntimeError("kl: unsupported memory layout")


class DistillKLFn(Function):
    """distill_kl / l2_loss(channel_wise=True) (other_loss.py:51-64, :67-76)."""

    @staticmethod
    def forward(ctx, ys, yt, T, eps_s, pad_zero_channel):
        _require_cuda(ys, yt)
        if ys.shape != yt.shape:
            raise RuntimeError("kl: shape mismatch")
        gs = _kl_strides(ys)
        if _kl_strides(yt) != gs:
            yt = yt.contiguous(memory_format=CL3D) if _is_cl3d(ys) else yt.contiguous()
            ys = ys if _kl_strides(ys) == _kl_strides(yt) else ys.contiguous()
            gs = _kl_strides(ys)
            if _kl_strides(yt) != gs:
                raise RuntimeError("kl: the two inputs must share a memory layout")
        N, C, V, sn, sc, sv = gs
        out = torch.empty((1,), dtype=torch.float32, device=ys.device)
        nb = query("mvd_kl_workspace_bytes", N, V)
        ws = _Workspace.get(nb, ys.device)
        if _is_bf16(ys) or _is_bf16(yt):
            # mixed precision: the bf16 NDHWC feature maps go into the kernel as they are (fp32 arithmetic inside)
            if not (_is_bf16(ys) and _is_bf16(yt) and _is_cl3d(ys) and (sc, sv, sn) == (1, C, V * C)) or pad_zero_channel:
                raise RuntimeError("kl: bf16 inputs must both be dense NDHWC feature maps")
            call("mvd_kl_fwd_bf16", _p(ys), _p(yt), _p(out), N, C, V, float(T), float(eps_s), _p(ws), ws.numel(), _stream())
            ctx.save_for_backward(ys, yt)
            ctx.cfg = (gs, float(T), float(eps_s), 0)
            return out.reshape(())
        call("mvd_kl_fwd", _p(ys), _p(yt), _p(out), N, C, V, sn, sc, sv, float(T), float(eps_s), int(pad_zero_channel),
             _p(ws), ws.numel(), _stream())
        ctx.save_for_backward(ys, yt)
        ctx.cfg = (gs, float(T), float(eps_s), int(pad_zero_channel))
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ys, yt = ctx.saved_tensors
        (N, C, V, sn, sc, sv), T, eps_s, pad = ctx.cfg
        g = g.contiguous()
        if _is_bf16(ys):
            gs = torch.empty_like(ys) if ctx.needs_input_grad[0] else None
            gt = torch.empty_like(yt) if ctx.needs_input_grad[1] else None
            call("mvd_kl_bwd_bf16", _p(ys), _p(yt), _p(g), 1.0, _p(gs), _p(gt), N, C, V, T, eps_s, _stream())
            return gs, gt, None, None, None
        # gradients are written with the inputs' strides into buffers of identical geometry
        def like(t):
            return torch.empty_strided(t.shape, t.stride(), dtype=torch.float32, device=t.device) \
                if (t.is_contiguous() or _is_cl3d(t)) else None
        gs = like(ys) if ctx.needs_input_grad[0] else None
        gt = like(yt) if ctx.needs_input_grad[1] else None
        dense = ys.is_contiguous() or _is_cl3d(ys)
        if not dense:
            # strided channel-slice view: write dense [N,C,V] grads (sn = C*V)
            if ctx.needs_input_grad[0]:
                gs = torch.empty(ys.shape, dtype=torch.float32, device=ys.device)
            if ctx.needs_input_grad[1]:
                gt = torch.empty(yt.shape, dtype=torch.float32, device=yt.device)
            ysd, ytd = ys.contiguous(), yt.contiguous()
            call("mvd_kl_bwd", _p(ysd), _p(ytd), _p(g), 1.0, _p(gs), _p(gt), N, C, V, C * V, V, 1, T, eps_s, pad, _stream())
        else:
            call("mvd_kl_bwd", _p(ys), _p(yt), _p(g), 1.0, _p(gs), _p(gt), N, C, V, sn, sc, sv, T, eps_s, pad, _stream())
        return gs, gt, None, None, None


class MseFn(Function):
    """l2_loss(channel_wise=False) = mean(|a - b|^2) (other_loss.py:77-78)."""

    @staticmethod
    def forward(ctx, a, b):
        _require_cuda(a, b)
        if a.shape != b.shape:
            raise RuntimeError("l2_loss: shape mismatch")
        if a.dtype != torch.float32 or b.dtype != torch.float32:
            raise RuntimeError("l2_loss: fp32 inputs (widen bf16 feature maps first)")
        # elementwise: both operands only have to share ONE dense layout (planar or NDHWC)
        if not (a.is_contiguous() or _is_cl3d(a)):
            a = a.contiguous()
        if a.stride() != b.stride():
            b = b.contiguous(memory_format=CL3D) if (_is_cl3d(a) and not a.is_contiguous()) else b.contiguous()
            if a.stride() != b.stride():
                a = a.contiguous()
                b = b.contiguous()
        # k_mse_fwd reads float4: a dense operand that does not start on a 16-byte boundary (a view into a larger buffer)
        # moves to an allocation of its own, strides kept
        a, b = (t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.preserve_format) for t in (a, b))
        n = a.numel()
        out = torch.empty((1,), dtype=torch.float32, device=a.device)
        ws = _Workspace.get(query("mvd_mse_workspace_bytes", n), a.device)
        call("mvd_mse_fwd", _p(a), _p(b), _p(out), n, _p(ws), ws.numel(), _stream())
        ctx.save_for_backward(a, b)
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        call("mvd_mse_bwd", _p(a), _p(b), _p(g), _p(ga), _p(gb), a.numel(), _stream())
        return ga, gb


class SoftmaxSelectFn(Function):
    """softmax(logits, 1)[:, sel:sel+1] on planar logits."""

    @staticmethod
    def forward(ctx, logits, sel):
        _require_cuda(logits)
        x = logits.contiguous()
        N, K = x.shape[:2]
        V = x[0, 0].numel()
        p = torch.empty((N, 1, *x.shape[2:]), dtype=torch.float32, device=x.device)
        call("mvd_softmax_select_fwd", _p(x), _p(p), N, V, K, int(sel), _stream())
        ctx.save_for_backward(x)
        ctx.sel = int(sel)
        return p

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        N, K = x.shape[:2]
        V = x[0, 0].numel()
        g = g.contiguous()
        dl = torch.empty_like(x)
        call("mvd_softmax_select_bwd", _p(x), _p(g), _p(dl), N, V, K, ctx.sel, _stream())
        return dl, None


def label_mask(labels, value):
    _require_cuda(labels)
    x = labels.contiguous().float()
    out = torch.empty_like(x)
    call("mvd_label_mask", _p(x), _p(out), x.numel(), float(value), _stream())
    return out


# ======================================================================================================== soft skeleton
def _vol(t):
    if t.dim() != 5:
        raise RuntimeError("soft-skeleton ops take [N,C,D,H,W] volumes")
    t = t.contiguous()
    N, C, D, H, W = t.shape
    return t, N * C, D, H, W


class SoftErodeFn(Function):
    @staticmethod
    def forward(ctx, x):
        _require_cuda(x)
        x, NC, D, H, W = _vol(x)
        y = torch.empty_like(x)
        code = torch.empty(x.shape, dtype=torch.int16, device=x.device) if x.requires_grad or True else None
        call("mvd_soft_erode_fwd", _p(x), _p(y), _p(code), NC, D, H, W, _stream())
        ctx.save_for_backward(code)
        ctx.dims = (NC, D, H, W)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (code,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        call("mvd_soft_erode_bwd", _p(code), _p(dy), _p(dx), *ctx.dims, _stream())
        return dx


class SoftDilateFn(Function):
    @staticmethod
    def forward(ctx, x):
        _require_cuda(x)
        x, NC, D, H, W = _vol(x)
        y = torch.empty_like(x)
        code = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        call("mvd_soft_dilate_fwd", _p(x), _p(y), _p(code), NC, D, H, W, _stream())
        ctx.save_for_backward(code)
        ctx.dims = (NC, D, H, W)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (code,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        call("mvd_soft_dilate_bwd", _p(code), _p(dy), _p(dx), *ctx.dims, _stream())
        return dx


class SkelUpdateFn(Function):
    """init: skel = relu(img - opened); else skel = skel + relu(delta - skel*delta) (soft_skeleton.py:31,35-36)."""

    @staticmethod
    def forward(ctx, img, opened, skel):
        _require_cuda(img, opened, skel)
        img, opened = img.contiguous(), opened.contiguous()
        init = skel is None
        if not init:
            skel = skel.contiguous()
        out = torch.empty_like(img)
        call("mvd_skel_update_fwd", _p(img), _p(opened), _p(skel), _p(out), img.numel(), int(init), _stream())
        ctx.save_for_backward(img, opened, skel)
        ctx.init = init
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        img, opened, skel = ctx.saved_tensors
        g = g.contiguous()
        d_img, d_open = torch.empty_like(img), torch.empty_like(img)
        d_skel = None if ctx.init else torch.empty_like(img)
        call("mvd_skel_update_bwd", _p(img), _p(opened), _p(skel), _p(g), _p(d_img), _p(d_open), _p(d_skel), img.numel(),
             int(ctx.init), _stream())
        return d_img, d_open, d_skel


def _skel_iter(img, skel, want_codes):
    """mvd_skel_iter_fwd on contiguous volumes; returns (e1 | None, opened, skel_out, c_e1 | None, c_e2, c_o)."""
    NC, D, H, W = img.shape[0] * img.shape[1], *img.shape[2:]
    init = skel is None
    e1 = None if init else torch.empty_like(img)
    opened, skel_out = torch.empty_like(img), torch.empty_like(img)
    c_e1 = torch.empty(img.shape, dtype=torch.int16, device=img.device) if (want_codes and not init) else None
    c_e2 = torch.empty(img.shape, dtype=torch.int16, device=img.device) if want_codes else None
    c_o = torch.empty(img.shape, dtype=torch.uint8, device=img.device) if want_codes else None
    call("mvd_skel_iter_fwd", _p(img), _p(skel), _p(e1), _p(opened), _p(skel_out), _p(c_e1), _p(c_e2), _p(c_o), NC, D, H, W,
         int(init), _stream())
    return e1, opened, skel_out, c_e1, c_e2, c_o


def _skel_iter_bwd_tail(x, opened, skel, c_e2, c_o, g, dims, init):
    """Shared backward of one fused step: (d e1 through the subtraction, d e1 through open(e1), d skel_in)."""
    d_a, d_o = torch.empty_like(x), torch.empty_like(x)
    d_skel = None if init else torch.empty_like(x)
    call("mvd_skel_update_bwd", _p(x), _p(opened), _p(skel), _p(g), _p(d_a), _p(d_o), _p(d_skel), x.numel(), int(init),
         _stream())
    d_e2 = torch.empty_like(x)
    call("mvd_soft_dilate_bwd", _p(c_o), _p(d_o), _p(d_e2), *dims, _stream())
    d_b = torch.empty_like(x)
    call("mvd_soft_erode_bwd", _p(c_e2), _p(d_e2), _p(d_b), *dims, _stream())
    return d_a, d_b, d_skel


class SkelInitFn(Function):
    """skel0 = relu(img - open(img)) (soft_skeleton.py:30-31) in one LDS-tiled launch."""

    @staticmethod
    def forward(ctx, img):
        _require_cuda(img)
        img, NC, D, H, W = _vol(img)
        need = ctx.needs_input_grad[0]
        _, opened, skel0, _, c_e2, c_o = _skel_iter(img, None, need)
        if need:
            ctx.save_for_backward(img, opened, c_e2, c_o)
        ctx.dims = (NC, D, H, W)
        return skel0

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        img, opened, c_e2, c_o = ctx.saved_tensors
        d_a, d_b, _ = _skel_iter_bwd_tail(img, opened, None, c_e2, c_o, g.contiguous(), ctx.dims, True)
        return d_a.add_(d_b)  # autograd's order: the subtraction's share first, then the share through open()


class SkelIterFn(Function):
    """(img, skel) -> (erode(img), skel + relu(d - skel*d)), d = relu(erode(img) - open(erode(img))): one iteration of
    the soft_skel loop (soft_skeleton.py:33-36) in one LDS-tiled launch."""

    @staticmethod
    def forward(ctx, img, skel):
        _require_cuda(img, skel)
        img, NC, D, H, W = _vol(img)
        skel = skel.contiguous()
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        e1, opened, skel_out, c_e1, c_e2, c_o = _skel_iter(img, skel, need)
        if need:
            ctx.save_for_backward(e1, opened, skel, c_e1, c_e2, c_o)
        ctx.dims = (NC, D, H, W)
        return e1, skel_out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_e1, d_skel_out):
        e1, opened, skel, c_e1, c_e2, c_o = ctx.saved_tensors
        g = d_skel_out.contiguous() if d_skel_out is not None else torch.zeros_like(e1)
        d_a, d_b, d_skel = _skel_iter_bwd_tail(e1, opened, skel, c_e2, c_o, g, ctx.dims, False)
        # e1's consumers in creation order: open(e1), the subtraction, the next iteration's erode -> autograd adds their
        # gradients in reverse: (next + subtraction) + open
        total = d_a if d_e1 is None else d_e1.contiguous() + d_a
        total = total.add_(d_b) if total is not d_a else d_a.add_(d_b)
        d_img = torch.empty_like(e1)
        call("mvd_soft_erode_bwd", _p(c_e1), _p(total), _p(d_img), *ctx.dims, _stream())
        return d_img, d_skel


class ClDiceFn(Function):
    """1 - 2*tprec*tsens/(tprec+tsens) from (skel_pred, target, skel_true, pred) (clDice_metric.py:7-36 formula)."""

    @staticmethod
    def forward(ctx, skel_pred, target, skel_true, pred, smooth):
        _require_cuda(skel_pred, target, skel_true, pred)
        sp, tg, st, pr = (t.contiguous() for t in (skel_pred, target, skel_true, pred))
        dev = sp.device
        n = sp.numel()
        sums = torch.empty((4,), dtype=torch.float32, device=dev)
        nb = query("mvd_dot_sum_workspace_bytes", n)
        ws = _Workspace.get(nb, dev)
        call("mvd_dot_sum", _p(sp), _p(tg), _p(sums), n, _p(ws), ws.numel(), _stream())
        call("mvd_dot_sum", _p(st), _p(pr), _p(sums[2:]), n, _p(ws), ws.numel(), _stream())
        out = torch.empty((5,), dtype=torch.float32, device=dev)
        call("mvd_cldice_combine", _p(sums), _p(out), float(smooth), _stream())
        ctx.save_for_backward(tg, st, out)
        return out[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        tg, st, out = ctx.saved_tensors
        # d/d skel_pred = g*(out1*target + out2); d/d pred = g*out3*skel_true  (tiny scalar glue on device)
        c = out * g
        d_sp = torch.addcmul(c[2].expand_as(tg), tg, c[1].expand_as(tg)) if ctx.needs_input_grad[0] else None
        d_pr = st * c[3] if ctx.needs_input_grad[3] else None
        return d_sp, None, None, d_pr, None


# ======================================================================================================== topology (integer)
def cc_label(mask, conn=6):
    """Connected components of a [D,H,W] uint8/bool mask: (int32 labels, int32 count tensor).  Canonical labels
    (1 + smallest linear index of the component) -> bit-exact against oracle/cc_oracle.c."""
    _require_cuda(mask)
    if mask.dim() != 3:
        raise RuntimeError("cc_label takes a [D,H,W] mask")
    m = mask.to(torch.uint8).contiguous()
    D, H, W = m.shape
    labels = torch.empty((D, H, W), dtype=torch.int32, device=m.device)
    count = torch.empty((1,), dtype=torch.int32, device=m.device)
    call("mvd_cc_label", _p(m), _p(labels), _p(count), D, H, W, int(conn), _stream())
    return labels, count


@functools.lru_cache(maxsize=None)
def _h0_slots(conn):
    """Key slots per vertex, from the library's own half-neighbourhood: the n offsets (dz, dy, dx), all in -1..1, give an
    L^3 grid sum (L - |dz|)(L - |dy|)(L - |dx|) edges, a number in (n (L-1)^3, n L^3]; for n <= 13 and L = 64 the
    intervals of different n are disjoint, so n = ceil(edges / L^3)."""
    return -(-query("mvd_h0_num_edges", 64, 64, 64, conn) // 64 ** 3)


def h0_persistence(f, conn=6, sublevel=True):
    """H0 persistence of a [D,H,W] device field: (birth [N], death [N], death_vertex [N]) as CPU tensors, one bar per
    vertex in linear-index order (the reference's C++ also returns its diagrams on the CPU, functional/sublevel.py:26-49).
    The filtration order of the edges comes from the device (edge keys + radix sort), the elder-rule pairing runs on
    the host (hom.cpp:51-69 restricted to vertices and edges)."""
    _require_cuda(f)
    if f.dim() != 3 or f.dtype != torch.float32:
        raise RuntimeError("h0_persistence takes a [D,H,W] float32 field")
    x = f.detach().contiguous()
    D, H, W = x.shape
    ne = query("mvd_h0_num_edges", D, H, W, int(conn))
    if ne < 0:
        raise RuntimeError("h0_persistence: conn must be 6, 14 or 26")
    nb = query("mvd_h0_workspace_bytes", D, H, W, int(conn))
    ws = _Workspace.get(nb, x.device)
    keys = torch.empty((D * H * W * _h0_slots(int(conn)),), dtype=torch.int64, device=x.device)
    call("mvd_h0_sorted_edges", _p(x), _p(keys), D, H, W, int(conn), int(bool(sublevel)), _p(ws), ws.numel(), _stream())
    keys_h = keys[:ne].cpu()          # synchronises the stream
    f_h = x.cpu()
    death = torch.empty((D * H * W,), dtype=torch.float32)
    dv = torch.empty((D * H * W,), dtype=torch.int64)
    ness = _lib.load().mvd_h0_pair_host(_p(f_h), _p(keys_h), ne, D, H, W, int(conn), int(bool(sublevel)), _p(death), _p(dv))
    if ness < 0:
        raise RuntimeError("mvd_h0_pair_host failed: " + _lib.load().mvd_last_error().decode())
    return f_h.reshape(-1), death, dv


class H0DiagramFn(Function):
    """Differentiable H0 diagram of a [D,H,W] field: returns a [N,2] CPU tensor of (birth, death) rows in vertex order,
    essential bars with death = +-inf, like dgms[0] of persistenceForwardHom (hom.cpp:155-185).  backward is the
    reference's persistence_backward (cohom.cpp:148-196): each finite diagram entry's gradient is added onto its critical
    vertex (birth -> the vertex itself, death -> the arg-max vertex of the killing edge), in diagram order."""

    @staticmethod
    def forward(ctx, f, conn, sublevel):
        birth, death, dv = h0_persistence(f, conn, sublevel)
        ctx.save_for_backward(dv)
        ctx.shape, ctx.device = tuple(f.shape), f.device
        return torch.stack([birth, death], 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (dv,) = ctx.saved_tensors
        g = g.detach().cpu().float()
        finite = dv >= 0
        grad = g[:, 0].clone()                                          # births: one bar per vertex (every bar has one)
        grad.index_add_(0, dv[finite], g[:, 1][finite])                 # deaths of the finite bars, in diagram order
        return grad.view(ctx.shape).to(ctx.device), None, None


# ------------------------------------------------------------------------- level-set persistence of 2-D images, H0 + H1
LS2D_MAX_K = 64
LS2D_HOST_THREADS = 16   # upper bound of the host pairing pool (never sized by the machine's core count)


def _ls2d_ints(vals):
    vals = [int(v) for v in vals]
    return (ctypes.c_int * len(vals))(*vals), len(vals)


def ls2d_num_cells(H, W, maxdim=1):
    """(n, V, E, T) of the Freudenthal triangulation of an [H, W] image (T = 0 for maxdim 0)."""
    nv, ne, nt = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    n = query("mvd_ls2d_num_cells", int(H), int(W), int(maxdim), ctypes.byref(nv), ctypes.byref(ne), ctypes.byref(nt))
    if n < 0:
        raise RuntimeError("levelset2d: H, W >= 1 and maxdim in (0, 1)")
    return n, nv.value, ne.value, nt.value


class _StageTimer:
    """Optional split of one "device keys + sort -> one D2H -> host pairing -> one H2D" round trip into the four times that
    `sink` (Ls2dTimes, Cub3dTimes) reports.  With `sink.on` false (the default) nothing is recorded and nothing waits.  Else
    the device stage is timed by two events, the host stages by the clock, and the stream is drained after the sort and
    after the H2D copy -- the two marks with device work in flight -- so that every stage is timed alone."""
    KEYS = ("keys_sort_ms", "d2h_ms", "host_sweep_ms", "h2d_ms")

    def __init__(self, sink):
        self.sink, self.on, self.t = sink, sink.on, []
        if self.on:
            self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            self.ev[0].record()

    def mark(self):
        """the end of the next stage of KEYS"""
        if not self.on:
            return
        if not self.t:
            self.ev[1].record()
        if len(self.t) in (0, 3):
            torch.cuda.current_stream().synchronize()
        self.t.append(time.perf_counter())

    def store(self, **extra):
        if self.on:
            ms = [self.ev[0].elapsed_time(self.ev[1])] + [(b - a) * 1e3 for a, b in zip(self.t, self.t[1:])]
            self.sink.last = dict(zip(self.KEYS, ms), **extra)


class Ls2dTimes:
    """Optional split of one levelset2d_persistence call (tools/bench_topoloss.py): set `Ls2dTimes.on = True`."""
    on = False
    last = None


def levelset2d_persistence(x, channels, sublevel, maxdim=1):
    """Dimension-0 and -1 level-set persistence of the planes (b, c), c in `channels`, of a [B,C,H,W] fp32 device tensor
    on the Freudenthal triangulation (LevelSetLayer2D of the reference, once per plane): P = B * len(channels) problems
    in one batch, problem p = b * len(channels) + j.  Device: keys + one merge sort per problem; one D2H copy; host: the
    elder-rule pairing of every problem (mvd_ls2d_pair_host); one H2D copy.
    Returns (bars, edge_row): DEVICE int32 tensors [P, V+T, 4] = (birth value bits, death value bits, birth critical vertex,
    death critical vertex) -- rows [0,V) dimension 0 in vertex order, rows [V,V+T) dimension 1 -- and [P, E]."""
    _require_cuda(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise RuntimeError("levelset2d_persistence takes a [B,C,H,W] float32 tensor")
    if maxdim not in (0, 1):
        raise RuntimeError("levelset2d_persistence: maxdim must be 0 or 1 (a 2-D image has no higher homology)")
    x = x.detach().contiguous()
    B, C, H, W = x.shape
    ch, nch = _ls2d_ints(channels)
    n, V, E, T = ls2d_num_cells(H, W, maxdim)
    P = B * nch
    nb = query("mvd_ls2d_workspace_bytes", P, H, W, int(maxdim))
    if nb == 0:
        raise RuntimeError(f"levelset2d_persistence: {P} problems of {W}x{H} do not fit one sort (2^31 cells)")
    ws = _Workspace.get(nb, x.device)
    keys = torch.empty((P, n), dtype=torch.int64, device=x.device)
    tm = _StageTimer(Ls2dTimes)
    call("mvd_ls2d_sorted_keys", _p(x), B, C, H, W, ch, nch, int(bool(sublevel)), int(maxdim), _p(keys), _p(ws), ws.numel(),
         _stream())
    tm.mark()
    keys_h = keys.cpu()               # the one D2H copy; synchronises the stream
    tm.mark()
    out_h = torch.empty((P * (V + T) * 4 + P * E,), dtype=torch.int32)
    bars_h, er_h = out_h[:P * (V + T) * 4], out_h[P * (V + T) * 4:]
    call("mvd_ls2d_pair_host", _p(keys_h), P, H, W, int(bool(sublevel)), int(maxdim), _p(bars_h), _p(er_h),
         LS2D_HOST_THREADS)
    tm.mark()
    out = out_h.to(x.device)          # the one H2D copy
    tm.mark()
    tm.store()
    return out[:P * (V + T) * 4].view(P, V + T, 4), out[P * (V + T) * 4:].view(P, E)


def _ls2d_dgms(bars, V):
    vals = bars[:, :, :2].view(torch.float32)
    return vals[:, :V].contiguous(), vals[:, V:].contiguous()


class LevelSetDiagram2DFn(Function):
    """Differentiable level-set diagrams of the planes (b, channels[j]) of x [B,C,H,W]: (dgm0 [P,V,2], dgm1 [P,T,2]) device
    tensors of (birth, death) rows in the sign of x (the flip of LevelSetLayer.forward for super-level undone), dgm0 in vertex
    order with the essential bar dying at +-inf, dgm1 in the order of the killing triangles.  maxdim 0 returns dgm0 alone.
    backward is the reference's persistence_backward (cohom.cpp:148-196): every finite entry's gradient is added onto its
    critical vertex -- as a gather per vertex in a fixed order, so the result is bit-identical from run to run."""

    @staticmethod
    def forward(ctx, x, channels, sublevel, maxdim=1):
        bars, edge_row = levelset2d_persistence(x, channels, sublevel, maxdim)
        B, C, H, W = x.shape
        ctx.save_for_backward(bars, edge_row)
        ctx.cfg = (B, C, H, W, [int(c) for c in channels], int(maxdim))
        dgm0, dgm1 = _ls2d_dgms(bars, H * W)
        return (dgm0, dgm1) if maxdim >= 1 else (dgm0,)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        bars, edge_row = ctx.saved_tensors
        B, C, H, W, channels, maxdim = ctx.cfg
        ch, nch = _ls2d_ints(channels)
        g0 = gs[0].contiguous().float()
        g1 = gs[1].contiguous().float() if maxdim >= 1 and bars.shape[1] > H * W else None
        grad = torch.empty((B, C, H, W), dtype=torch.float32, device=bars.device)
        call("mvd_ls2d_diagram_bwd", _p(g0), _p(g1), _p(bars), _p(edge_row), B, C, H, W, ch, nch,
             maxdim if g1 is not None else 0, _p(grad), _stream())
        return grad, None, None, None


def _ls2d_check_k(k):
    if not 1 <= int(k) <= LS2D_MAX_K:
        raise ValueError(f"top-k bar lengths: k must be in 1..{LS2D_MAX_K} (got {k}); the selection kernel holds one "
                         f"problem's bars of both endpoints in one workgroup")
    return int(k)


def ls2d_topk(bars, H, W, maxdim, sublevel, k):
    """(lengths [P,2,k] fp32, index [P,2,k] int32) of the k longest bars per problem and dimension, descending."""
    k = _ls2d_check_k(k)
    P = bars.shape[0]
    lengths = torch.empty((P, 2, k), dtype=torch.float32, device=bars.device)
    index = torch.empty((P, 2, k), dtype=torch.int32, device=bars.device)
    call("mvd_ls2d_topk", _p(bars), P, int(H), int(W), int(maxdim), int(bool(sublevel)), k, _p(lengths), _p(index), _stream())
    return lengths, index


class TopKBarLengths2DFn(Function):
    """TopKBarcodeLengths (nn/features.py:128-150) of batched diagrams dgm0 [P,V,2] / dgm1 [P,T,2]: [P,k] lengths of
    dimension `dim`.  `size` = (W, H) of the image the diagrams come from."""

    @staticmethod
    def forward(ctx, dgm, dim, k, sublevel):
        _require_cuda(dgm)
        if dgm.dim() != 3 or dgm.shape[2] != 2 or dgm.dtype != torch.float32:
            raise RuntimeError("top-k bar lengths take a [P,n,2] float32 diagram")
        k = _ls2d_check_k(k)
        P, n = dgm.shape[:2]
        # the kernel's bar layout with this diagram alone as a 1 x n "image" of dimension 0 (vertex columns unused)
        bars = torch.zeros((P, n, 4), dtype=torch.int32, device=dgm.device)
        bars[:, :, :2] = dgm.detach().contiguous().view(torch.int32)
        lengths, index = ls2d_topk(bars, 1, n, 0, sublevel, k)
        ctx.save_for_backward(index)
        ctx.cfg = (P, n, k, bool(sublevel))
        return lengths[:, 0].contiguous()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (index,) = ctx.saved_tensors
        P, n, k, sublevel = ctx.cfg
        gl = torch.zeros((P, 2, k), dtype=torch.float32, device=g.device)
        gl[:, 0] = g
        gb = torch.empty((P, n, 2), dtype=torch.float32, device=g.device)
        call("mvd_ls2d_topk_bwd", _p(gl), _p(index), P, 1, n, 0, int(sublevel), k, _p(gb), _stream())
        return gb, None, None, None


class TopoLossFn(Function):
    """l_topo of TopoLoss.forward (loss/Topo_Loss.py:39-41,49-85) summed over `idx`: for every sample b and class i in idx the
    super-level diagram of y_pred[b, i+1], its max_k longest bars per dimension squared, the first label[b,i,dim] of them
    signed -1, the mean over the batch.  ONE batch of B * len(idx) problems -> one host round trip in the forward, none in
    the backward, which writes grad y_pred directly."""

    @staticmethod
    def forward(ctx, y_pred, topo_label, idx, max_k):
        _require_cuda(y_pred, topo_label)
        k = _ls2d_check_k(max_k)
        if y_pred.dim() != 4 or y_pred.dtype != torch.float32:
            raise RuntimeError("TopoLoss takes y_pred [B,C,H,W] float32 (the reference's layer is 2-D)")
        B, C, H, W = y_pred.shape
        idx = [int(i) for i in idx]
        if topo_label.dim() != 3 or topo_label.shape[0] != B or topo_label.shape[2] != 2 or topo_label.is_floating_point():
            raise RuntimeError(f"TopoLoss: topo_label must be an integer [B={B}, C, 2] tensor")
        n_label = topo_label.shape[1]
        if not idx or min(idx) < 0 or max(idx) >= n_label or max(idx) + 1 >= C or len(set(idx)) != len(idx):
            raise RuntimeError(f"TopoLoss: idx {idx} must be distinct classes with a row in topo_label ({n_label}) and a channel "
                               f"idx+1 in y_pred ({C})")
        label = topo_label.to(torch.int32).contiguous()
        bars, _ = levelset2d_persistence(y_pred, [i + 1 for i in idx], False, 1)
        lengths, index = ls2d_topk(bars, H, W, 1, False, k)
        ci, ni = _ls2d_ints(idx)
        out = torch.empty((1,), dtype=torch.float32, device=y_pred.device)
        call("mvd_ls2d_topoloss_fwd", _p(lengths), _p(label), B, ci, ni, n_label, k, _p(out), _stream())
        ctx.save_for_backward(lengths, index, bars, label)
        ctx.cfg = (B, C, H, W, idx, n_label, k)
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lengths, index, bars, label = ctx.saved_tensors
        B, C, H, W, idx, n_label, k = ctx.cfg
        ci, ni = _ls2d_ints(idx)
        g = g.contiguous().float()
        grad = torch.empty((B, C, H, W), dtype=torch.float32, device=g.device)
        call("mvd_ls2d_topoloss_bwd", _p(lengths), _p(index), _p(bars), _p(label), _p(g), B, C, H, W, ci, ni, n_label, k, 0,
             _p(grad), _stream())
        return grad, None, None, None


def ls2d_betti_numbers(target, num_classes):
    """int32 [B, num_classes, 2]: (beta0, beta1) of every class's binary mask of a [B,1,H,W] / [B,H,W] label map = the bars
    of non-zero length of the mask's super-level diagram (the essential dimension-0 bar closed at the floor 0)."""
    _require_cuda(target)
    t = target
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3:
        raise RuntimeError("betti_topo_label takes a [B,1,H,W] or [B,H,W] label map")
    B, H, W = t.shape
    t = t.to(torch.float32).contiguous()
    C = int(num_classes)
    planes = torch.empty((B, C, H, W), dtype=torch.float32, device=t.device)
    call("mvd_ls2d_onehot", _p(t), _p(planes), B, C, H * W, _stream())
    bars, _ = levelset2d_persistence(planes, list(range(C)), False, 1)
    counts = torch.empty((B * C, 2), dtype=torch.int32, device=t.device)
    call("mvd_ls2d_count_bars", _p(bars), B * C, H, W, 0, _p(counts), _stream())
    return counts.view(B, C, 2)


# ------------------------------------------------------------------------- 3-D cubical persistence, dimensions 0 and 2
CUB3D_HOST_THREADS = 16   # upper bound of the host pairing pool (never sized by the machine's core count)


class Cub3dTimes:
    """Optional split of one cubical loss step (tools/bench_cubical_topo.py): set `Cub3dTimes.on = True`."""
    on = False
    last = None


def cub3d_check_dim(dim):
    if int(dim) == 1:
        raise NotImplementedError("3-D cubical persistence of dimension 1 needs a boundary-matrix reduction; dimensions 0 and 2 "
                                  "reduce to union-find and are the ones built")
    if int(dim) not in (0, 2):
        raise ValueError(f"3-D cubical persistence: dimension must be 0 or 2 (got {dim})")
    return int(dim)


def _cub3d_field(field):
    _require_cuda(field)
    if field.dim() != 4 or field.dtype != torch.float32:
        raise RuntimeError("3-D cubical persistence takes a [N,D,H,W] float32 field")
    x = field.detach().contiguous()
    if x.numel() == 0:
        raise RuntimeError("3-D cubical persistence: empty field")
    if bool(torch.isnan(x).any()):
        raise ValueError("3-D cubical persistence: the field contains NaN (a filtration needs a total order)")
    return x


def _cub3d_bars(x, dim):
    """(bars [n_total,2] int32 device, offsets int32 numpy [N+1], offsets on the device) of a checked field x [N,D,H,W]:
    device keys + one radix sort per sample, one D2H copy, the host sweep (mvd_cub3d_pair_host), one H2D copy."""
    N, D, H, W = x.shape
    V = D * H * W
    nv = ctypes.c_long()
    slots = query("mvd_cub3d_num_keys", D, H, W, dim, ctypes.byref(nv))
    nb = query("mvd_cub3d_workspace_bytes", D, H, W, dim)
    if slots < 0 or nb == 0:
        raise RuntimeError(f"3-D cubical persistence: a {D}x{H}x{W} grid does not fit one sort (2^31 edge slots)")
    nv = nv.value
    ws = _Workspace.get(nb, x.device)
    keys = torch.empty((N, slots), dtype=torch.int64, device=x.device)
    tm = _StageTimer(Cub3dTimes)
    call("mvd_cub3d_sorted_keys", _p(x), N, D, H, W, dim, _p(keys), _p(ws), ws.numel(), _stream())
    tm.mark()
    keys_h = keys[:, :nv].cpu()       # synchronises the stream
    f_h = x.cpu()
    tm.mark()
    bars_h = torch.empty((N, V, 2), dtype=torch.int32)
    counts = torch.empty((N,), dtype=torch.int32)
    call("mvd_cub3d_pair_host", _p(f_h), _p(keys_h), nv, N, D, H, W, dim, _p(bars_h), _p(counts), CUB3D_HOST_THREADS)
    tm.mark()
    cnt = counts.numpy().astype(np.int64)
    offsets = np.zeros(N + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(cnt)
    packed = torch.cat([bars_h[n, :int(cnt[n])] for n in range(N)]) if N > 1 else bars_h[0, :int(cnt[0])]
    bars = packed.contiguous().to(x.device)
    offsets_dev = torch.from_numpy(offsets).to(x.device)
    tm.mark()
    tm.store(bars=int(offsets[-1]))
    return bars, offsets, offsets_dev


def cubical3d_persistence(field, dim):
    """Bars of non-zero length of the dimension-`dim` (0 or 2) sublevel cubical persistence of every sample of a
    [N,D,H,W] fp32 device field, voxels as top-dimensional cells: a list of N device int32 tensors [n,2] of unpadded linear
    voxel indices (birth voxel, death voxel) -- the bar is (f[birth voxel], f[death voxel]).  Essential bars are dropped."""
    dim = cub3d_check_dim(dim)
    bars, offsets, _ = _cub3d_bars(_cub3d_field(field), dim)
    return [bars[int(offsets[n]):int(offsets[n + 1])] for n in range(field.shape[0])]


def _cub3d_plan(x, bars, offsets_dev, selected, n_total):
    N, V = x.shape[0], x[0].numel()
    ws = _Workspace.get(query("mvd_cub3d_match_workspace_bytes", n_total), x.device)
    key = torch.empty((2 * n_total,), dtype=torch.int32, device=x.device)
    order = torch.empty((2 * n_total,), dtype=torch.int32, device=x.device)
    call("mvd_cub3d_scatter_plan", _p(x), _p(bars), _p(offsets_dev), _p(selected), N, V, n_total, _p(key), _p(order), _p(ws),
         ws.numel(), _stream())
    return key, order


class CubicalDiagram3DFn(Function):
    """Differentiable diagram of dimension `dim` of field [N,D,H,W]: (dgm [n_total,2] fp32 of (birth, death) rows gathered
    from the field, offsets [N+1]): sample n owns rows [offsets[n], offsets[n+1]).  backward adds every entry's gradient onto
    its voxel -- one thread per voxel run in a fixed order, bit-identical from run to run."""

    @staticmethod
    def forward(ctx, field, dim):
        dim = cub3d_check_dim(dim)
        x = _cub3d_field(field)
        bars, offsets, offsets_dev = _cub3d_bars(x, dim)
        N, V = x.shape[0], x[0].numel()
        base = torch.repeat_interleave(torch.arange(N, device=x.device, dtype=torch.int64) * V,
                                       torch.from_numpy(np.diff(offsets).astype(np.int64)).to(x.device))
        dgm = x.reshape(-1)[bars.to(torch.int64) + base[:, None]]
        ctx.save_for_backward(x, bars, offsets_dev)
        ctx.shape = tuple(field.shape)
        off_t = torch.from_numpy(offsets.astype(np.int64))
        ctx.mark_non_differentiable(off_t)
        return dgm, off_t

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        x, bars, offsets_dev = ctx.saved_tensors
        N, V, n_total = x.shape[0], x[0].numel(), bars.shape[0]
        grad = torch.empty(ctx.shape, dtype=torch.float32, device=x.device)
        key = order = None
        if n_total:
            key, order = _cub3d_plan(x, bars, offsets_dev, None, n_total)
        call("mvd_cub3d_diagram_bwd", _p(g.contiguous().float()), _p(key), _p(order), N, V, n_total, _p(grad), _stream())
        return grad, None


def cubical3d_target_count(target, dim):
    """m [N] int32 on the device: the number of points (0, 1) of the dimension-`dim` diagram of a binary [N,D,H,W] mask."""
    dim = cub3d_check_dim(dim)
    _require_cuda(target)
    if target.dim() != 4:
        raise RuntimeError("cubical3d_target_count takes a [N,D,H,W] mask")
    t = target.detach().to(torch.float32).contiguous()
    N, D, H, W = t.shape
    ws = _Workspace.get(query("mvd_cub3d_target_workspace_bytes", D, H, W), t.device)
    m = torch.empty((N,), dtype=torch.int32, device=t.device)
    call("mvd_cub3d_target_count", _p(t), N, D, H, W, dim, _p(m), _p(ws), ws.numel(), _stream())
    return m


class CubicalWassersteinFn(Function):
    """mean over the batch of the q-Wasserstein distance (L-inf ground metric, the diagonal allowed) between the
    dimension-`dim` cubical diagram of field [N,D,H,W] and the diagram of the binary target mask [N,D,H,W], m copies of (0, 1).
    Against m identical points the optimal matching is the selection of the <= m bars of largest positive gain
    c0^q + 2^-q - c1^q, so no assignment problem is solved.  One host round trip (the pairing sweep) in the forward, none in
    the backward, which is one memset and one launch."""

    @staticmethod
    def forward(ctx, field, target, dim, q):
        dim = cub3d_check_dim(dim)
        q = float(q)
        if not q >= 1.0:
            raise ValueError(f"Wasserstein exponent q must be >= 1 (got {q})")
        x = _cub3d_field(field)
        if tuple(target.shape) != tuple(x.shape):
            raise RuntimeError(f"cubical Wasserstein loss: field {tuple(x.shape)} and target {tuple(target.shape)} differ")
        m = cubical3d_target_count(target, dim)
        bars, offsets, offsets_dev = _cub3d_bars(x, dim)
        timed = Cub3dTimes.on
        if timed:
            t0 = time.perf_counter()
        N, V, n_total = x.shape[0], x[0].numel(), int(offsets[-1])
        ws = _Workspace.get(query("mvd_cub3d_match_workspace_bytes", n_total), x.device)
        selected = torch.empty((max(n_total, 1),), dtype=torch.uint8, device=x.device)
        wq = torch.empty((N,), dtype=torch.float64, device=x.device)
        out = torch.empty((1,), dtype=torch.float32, device=x.device)
        call("mvd_cub3d_match_fwd", _p(x), _p(bars), ctypes.c_void_p(offsets.ctypes.data), _p(offsets_dev), _p(m), N, V, q,
             _p(selected), _p(wq), _p(out), _p(ws), ws.numel(), _stream())
        key = order = None
        if n_total and ctx.needs_input_grad[0]:
            key, order = _cub3d_plan(x, bars, offsets_dev, selected, n_total)
        if timed:
            torch.cuda.synchronize()
            Cub3dTimes.last["match_loss_ms"] = (time.perf_counter() - t0) * 1e3
        ctx.save_for_backward(x, bars, offsets_dev, selected, wq, key, order)
        ctx.cfg = (q, tuple(field.shape))
        ctx.mark_non_differentiable(m)
        return out.reshape(()), m

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        x, bars, offsets_dev, selected, wq, key, order = ctx.saved_tensors
        q, shape = ctx.cfg
        N, V, n_total = x.shape[0], x[0].numel(), bars.shape[0]
        grad = torch.empty(shape, dtype=torch.float32, device=x.device)
        g = g.reshape(1).contiguous().float()
        call("mvd_cub3d_match_bwd", _p(x), _p(bars), _p(offsets_dev), _p(selected), _p(wq), _p(g), _p(key), _p(order), N, V,
             n_total, q, _p(grad), _stream())
        return grad, None, None, None


def threshold_mask(f, thr, ge=False):
    _require_cuda(f)
    x = f.contiguous()
    m = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    call("mvd_threshold_mask", _p(x), _p(m), x.numel(), float(thr), int(ge), _stream())
    return m


def seg_label_mask(seg, labels):
    """uint8 mask of the voxels of an int32 segmentation whose label is in `labels` (1..16 ints)."""
    _require_cuda(seg)
    if seg.dtype != torch.int32:
        raise RuntimeError("seg_label_mask takes an int32 segmentation")
    x = seg.contiguous()
    ls = (ctypes.c_int32 * len(labels))(*[int(v) for v in labels])
    m = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    call("mvd_seg_label_mask", _p(x), _p(m), x.numel(), ctypes.cast(ls, ctypes.c_void_p), len(labels), _stream())
    return m


def cc_keep_largest(cc_labels, keep=2):
    """int32[4] device tensor {label0, label1, size0, size1} of the `keep` largest components of a canonical
    label volume (ties -> smaller label)."""
    _require_cuda(cc_labels)
    x = cc_labels.contiguous()
    n = x.numel()
    ws = torch.empty((query("mvd_cc_keep_workspace_bytes", n),), dtype=torch.uint8, device=x.device)
    kept = torch.empty((4,), dtype=torch.int32, device=x.device)
    call("mvd_cc_keep_largest", _p(x), n, int(keep), _p(kept), _p(ws), _stream())
    return kept


def seg_remove_components(seg, cc_labels, kept, background=0):
    _require_cuda(seg)
    x = seg.contiguous()
    out = torch.empty_like(x)
    call("mvd_seg_remove_components", _p(x), _p(cc_labels.contiguous()), _p(kept), _p(out), x.numel(),
         int(background), _stream())
    return out


# ------------------------------------------------------------------------------------------------ attention (csrc/attention.hip)
# The bottleneck fusion block of FinalNetv2: tokens are the [B, N, C] memory of an NDHWC bottleneck.  `drop` is None (no
# dropout: eval mode, or p = 0) or (state, p, site): the module's device buffer {seed, t}, the probability and the site
# number that keys the Philox stream (header: mvd_dropout_*).
ATTN_MAX_TOKENS = 256
ATTN_HEAD_DIMS = (4, 64)   # dh in [4, 64], a multiple of 4


def _drop3(drop):
    if drop is None or not drop[1] > 0:
        return None, 0.0, 0
    state, p, site = drop
    if not (state.is_cuda and state.dtype == torch.int64 and state.numel() == 2):
        raise RuntimeError("dropout state must be a cuda int64 tensor {seed, t}")
    return _p(state), float(p), int(site)


def _f32c(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("attention ops take contiguous fp32 cuda tensors (the fusion block is fp32 only)")


def dropout_tick(state):
    """t += 1 in the device state {seed, t}: once at the head of a training-mode forward."""
    _require_cuda(state)
    call("mvd_dropout_tick", _p(state), _stream())


def dropout_mask(seed, t, site, p, n, device):
    """The keep mask (uint8, 1 = kept) of elements 0..n-1 of (seed, t, site): what the kernels regenerate (tests)."""
    out = torch.empty(int(n), dtype=torch.uint8, device=device)
    call("mvd_dropout_mask", int(seed), int(t), int(site), float(p), int(n), _p(out), _stream())
    return out


def layernorm_fwd(x, gamma, beta, eps, pos=None, want_sum=True):
    """x [..., C] -> (y, xs, mean, rstd); with `pos` ([1, N, C] or [N, C]) xs = x + pos is what gets normalised (and is
    returned for the residuals), else xs is x."""
    _f32c(x, gamma, beta, pos)
    C = x.shape[-1]
    M = x.numel() // C
    y = torch.empty_like(x)
    xs = torch.empty_like(x) if pos is not None and want_sum else None
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    npos = pos.numel() // C if pos is not None else 0
    call("mvd_layernorm_fwd", _p(x), _p(pos), _p(xs), _p(y), _p(mean), _p(rstd), _p(gamma), _p(beta), M, C, npos, float(eps),
         _stream())
    return y, (xs if pos is not None else x), mean, rstd


def layernorm_bwd(dy, xs, mean, rstd, gamma, dres1=None, dres2=None, npos=0, drop=None, dgamma=None, dbeta=None, dpos=None):
    """-> (dx, dxd, dgamma, dbeta, dpos): dx includes the residual gradients dres1 / dres2; dxd (with `drop`) is dx times
    the dropout factors of `drop`'s site; dpos ([npos, C], with npos > 0) sums dx over the batch."""
    _f32c(dy, xs, gamma, dres1, dres2, dgamma, dbeta, dpos)
    C = xs.shape[-1]
    M = xs.numel() // C
    dev = xs.device
    dx = torch.empty_like(xs)
    st, p, site = _drop3(drop)
    dxd = torch.empty_like(xs) if drop is not None else None
    dgamma = dgamma if dgamma is not None else torch.empty(C, dtype=torch.float32, device=dev)
    dbeta = dbeta if dbeta is not None else torch.empty(C, dtype=torch.float32, device=dev)
    if npos and dpos is None:
        dpos = torch.empty((npos, C), dtype=torch.float32, device=dev)
    call("mvd_layernorm_bwd", _p(dy), _p(xs), _p(mean), _p(rstd), _p(gamma), _p(dres1), _p(dres2), _p(dx), _p(dxd), _p(dgamma),
         _p(dbeta), _p(dpos) if npos else None, M, C, int(npos), st, p, site, _stream())
    return dx, dxd, dgamma, dbeta, (dpos if npos else None)


def linear_fwd(x, w, bias=None, res=None, drop=None):
    """y[..., O] = (x[..., C] w[O, C]^T + bias) * dropout + res: torch's nn.Linear weight itself, MFMA fp32."""
    _f32c(x, w, bias, res)
    O, C = w.shape
    M = x.numel() // C
    y = torch.empty(tuple(x.shape[:-1]) + (O,), dtype=torch.float32, device=x.device)
    st, p, site = _drop3(drop)
    call("mvd_linear_fwd", _p(x), _p(w), _p(bias), _p(res), _p(y), M, C, O, st, p, site, _stream())
    return y


def linear_bwd(g, x, w, need_dx=True, dw=None, db=None, has_bias=False):
    """g = dy (times the dropout factors, where the forward dropped) -> (dx, dw, db); dw / db may be given (gradient sinks)."""
    _f32c(g, x, w, dw, db)
    O, C = w.shape
    M = x.numel() // C
    dev = x.device
    dx = torch.empty_like(x) if need_dx else None
    dw = dw if dw is not None else torch.empty((O, C), dtype=torch.float32, device=dev)
    if has_bias and db is None:
        db = torch.empty(O, dtype=torch.float32, device=dev)
    call("mvd_linear_bwd", _p(g), _p(x), _p(w), _p(dx), _p(dw), _p(db) if has_bias else None, M, C, O, _stream())
    return dx, dw, (db if has_bias else None)


def _attn_dims(qbuf, heads):
    B, N, C3 = qbuf.shape
    C = C3 // 3
    if C3 != 3 * C or C % heads:
        raise RuntimeError(f"attention: a [B, N, 3C] qkv buffer with C a multiple of {heads} heads is needed, got {tuple(qbuf.shape)}")
    return B, N, C, C // heads


def attention_fwd(qbuf, kvbuf, heads, res=None, drop=None):
    """out[B, N, C] = dropout(softmax(q k^T / sqrt(dh))) v [+ res]; q from qbuf, k and v from kvbuf ([B, N, 3C], read in
    place through the head stride).  -> (out, rowmax, rowsum)"""
    _f32c(qbuf, kvbuf, res)
    B, N, C, dh = _attn_dims(qbuf, heads)
    if kvbuf.shape != qbuf.shape:
        raise RuntimeError("attention: the two qkv buffers differ in shape")
    out = torch.empty((B, N, C), dtype=torch.float32, device=qbuf.device)
    rowmax = torch.empty(B * heads * N, dtype=torch.float32, device=qbuf.device)
    rowsum = torch.empty_like(rowmax)
    st, p, site = _drop3(drop)
    call("mvd_attention_fwd", _p(qbuf), _p(kvbuf), _p(res), _p(out), _p(rowmax), _p(rowsum), B, N, heads, dh, st, p, site,
         _stream())
    return out, rowmax, rowsum


def attention_bwd(qbuf, kvbuf, dout, rowmax, rowsum, heads, dqbuf, dkvbuf, drop=None):
    """dq into dqbuf's q section, dk / dv into dkvbuf's k / v sections (both [B, N, 3C]; one buffer for self-attention)."""
    _f32c(qbuf, kvbuf, dout, dqbuf, dkvbuf)
    B, N, C, dh = _attn_dims(qbuf, heads)
    delta = torch.empty_like(rowmax)
    st, p, site = _drop3(drop)
    call("mvd_attention_bwd", _p(qbuf), _p(kvbuf), _p(dout), _p(rowmax), _p(rowsum), _p(delta), _p(dqbuf), _p(dkvbuf), B, N,
         heads, dh, st, p, site, _stream())


def mean2(a, b):
    """(a + b) / 2 of two logits tensors (FinalNetv2 without deep supervision, selfattnNet.py:944); inference only."""
    _require_cuda(a, b)
    if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
        raise RuntimeError("mean2 has no backward: the averaged output of FinalNetv2 is its inference output (torch.no_grad())")
    a, b = a.contiguous(), b.contiguous()
    out = torch.zeros_like(a)
    call("mvd_axpy", _p(out), _p(a), 0.5, a.numel(), _stream())
    call("mvd_axpy", _p(out), _p(b), 0.5, a.numel(), _stream())
    return out


def _sink(param, shape, dev):
    """(tensor the gradient kernel writes, what goes back to autograd): the parameter's flat-buffer slice and None when the
    optimizer offers one (optim.FlatParams), else a fresh tensor twice."""
    t = _take_grad(param)
    if t is not None:
        return t, None
    t = torch.empty(shape, dtype=torch.float32, device=dev)
    return t, t


class LayerNormFn(Function):
    """nn.LayerNorm(C) over the last axis."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x = x.contiguous()
        y, _, mean, rstd = layernorm_fwd(x, gamma.detach(), beta.detach(), eps)
        ctx.save_for_backward(x, mean, rstd, gamma.detach())
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, mean, rstd, gamma = ctx.saved_tensors
        dx, _, dg, db, _ = layernorm_bwd(dy.contiguous(), x, mean, rstd, gamma)
        return dx, dg, db, None


class TokenLinearFn(Function):
    """nn.Linear on tokens: y = x W^T (+ b)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        ctx.save_for_backward(x, weight.detach())
        ctx.has_bias = bias is not None
        return linear_fwd(x, weight.detach(), bias.detach() if bias is not None else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx, dw, db = linear_bwd(dy.contiguous(), x, w, need_dx=ctx.needs_input_grad[0], has_bias=ctx.has_bias)
        return dx, dw, db


class AttentionFn(Function):
    """Multi-head attention without dropout over two [B, N, 3C] qkv buffers (queries of the first, keys / values of the
    second)."""

    @staticmethod
    def forward(ctx, qbuf, kvbuf, heads):
        qbuf, kvbuf = qbuf.contiguous(), kvbuf.contiguous()
        out, rowmax, rowsum = attention_fwd(qbuf, kvbuf, heads)
        ctx.save_for_backward(qbuf, kvbuf, rowmax, rowsum)
        ctx.heads = heads
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qbuf, kvbuf, rowmax, rowsum = ctx.saved_tensors
        dq, dkv = torch.zeros_like(qbuf), torch.zeros_like(kvbuf)   # (the sections the other buffer owns stay 0)
        attention_bwd(qbuf, kvbuf, dout.contiguous(), rowmax, rowsum, ctx.heads, dq, dkv)
        return dq, dkv, None


# dropout sites of the fusion block (the six nn.Dropout calls that act in FinalNetv2.forward)
SITE_ATTN1, SITE_ATTN2, SITE_PROJ1, SITE_PROJ2, SITE_SELF1, SITE_SELF2 = range(6)
FUSION_PARAMS = ("pos1", "pos2", "n1w", "n1b", "n2w", "n2b", "n3w", "n3b", "n4w", "n4b", "qkv1", "qkv2", "p1w", "p1b", "p2w",
                 "p2b", "sa1", "sa2")


class BottleneckFusionFn(Function):
    """selfattnNet.py:917-939 on two NDHWC bottlenecks [B, C, D, H, W] (tokens = voxels in raster order: a view):
        xs1 = x1 + pos1, xs2 = x2 + pos2
        a1 = drop(proj1(attn(q of qkv1(norm1 xs2), k / v of qkv2(norm2 xs1)))) + xs2,  a2 = the mirror image + xs1
        y1 = xs1 + attn(qkv_sa1(norm3 a1)),  y2 = xs2 + attn(qkv_sa2(norm4 a2))
    14 launches forward (+ 1 in training: the step counter), 24 backward; residual sums and the proj dropout's backward
    ride in the producing kernels."""

    @staticmethod
    def forward(ctx, x1, x2, state, heads, p_attn, p_proj, training, eps, *params):
        P = dict(zip(FUSION_PARAMS, [q.detach() for q in params]))
        x1, x2 = to_ndhwc(x1), to_ndhwc(x2)
        if x1.dtype != torch.float32 or x2.dtype != torch.float32:
            raise RuntimeError("the bottleneck fusion block is fp32 only")
        B, C = x1.shape[:2]
        N = x1[0, 0].numel()
        t1, t2 = x1.permute(0, 2, 3, 4, 1).reshape(B, N, C), x2.permute(0, 2, 3, 4, 1).reshape(B, N, C)   # views
        if training:
            dropout_tick(state)
        d = (lambda p, site: (state, p, site) if (training and p > 0) else None)
        ctx.drops = {s: d(p_attn if s in (SITE_ATTN1, SITE_ATTN2, SITE_SELF1, SITE_SELF2) else p_proj, s) for s in range(6)}
        n2x1, xs1, m2, r2 = layernorm_fwd(t1, P["n2w"], P["n2b"], eps, P["pos1"])
        n1x2, xs2, m1, r1 = layernorm_fwd(t2, P["n1w"], P["n1b"], eps, P["pos2"])
        qkv1 = linear_fwd(n1x2, P["qkv1"])
        qkv2 = linear_fwd(n2x1, P["qkv2"])
        o1, mx1, sm1 = attention_fwd(qkv1, qkv2, heads, None, ctx.drops[SITE_ATTN1])
        o2, mx2, sm2 = attention_fwd(qkv2, qkv1, heads, None, ctx.drops[SITE_ATTN2])
        a1 = linear_fwd(o1, P["p1w"], P["p1b"], xs2, ctx.drops[SITE_PROJ1])
        a2 = linear_fwd(o2, P["p2w"], P["p2b"], xs1, ctx.drops[SITE_PROJ2])
        n3, _, m3, r3 = layernorm_fwd(a1, P["n3w"], P["n3b"], eps)
        n4, _, m4, r4 = layernorm_fwd(a2, P["n4w"], P["n4b"], eps)
        qkv3 = linear_fwd(n3, P["sa1"])
        qkv4 = linear_fwd(n4, P["sa2"])
        y1, mx3, sm3 = attention_fwd(qkv3, qkv3, heads, xs1, ctx.drops[SITE_SELF1])
        y2, mx4, sm4 = attention_fwd(qkv4, qkv4, heads, xs2, ctx.drops[SITE_SELF2])
        ctx.save_for_backward(xs1, xs2, m1, r1, m2, r2, n1x2, n2x1, qkv1, qkv2, o1, o2, mx1, sm1, mx2, sm2, a1, a2, m3, r3, m4,
                              r4, n3, n4, qkv3, qkv4, mx3, sm3, mx4, sm4, *P.values())
        ctx.params = params
        ctx.heads, ctx.geom = heads, (B, N, C)
        ctx.sp = sp = tuple(x1.shape)
        as5 = lambda y: y.view(B, *sp[2:], C).permute(0, 4, 1, 2, 3)   # [B, N, C] memory as NDHWC [B, C, D, H, W]
        return as5(y1), as5(y2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy1, dy2):
        sv = ctx.saved_tensors
        (xs1, xs2, m1, r1, m2, r2, n1x2, n2x1, qkv1, qkv2, o1, o2, mx1, sm1, mx2, sm2, a1, a2, m3, r3, m4, r4, n3, n4, qkv3, qkv4,
         mx3, sm3, mx4, sm4) = sv[:30]
        P = dict(zip(FUSION_PARAMS, sv[30:]))
        prm = dict(zip(FUSION_PARAMS, ctx.params))
        B, N, C = ctx.geom
        H, dr, dev = ctx.heads, ctx.drops, xs1.device
        tok = lambda g: to_ndhwc(g).permute(0, 2, 3, 4, 1).reshape(B, N, C)
        dy1, dy2 = tok(dy1), tok(dy2)
        sink, ret = {}, {}
        for k in FUSION_PARAMS:
            sink[k], ret[k] = _sink(prm[k], tuple(prm[k].shape), dev)
        # the two self-attentions and their qkv linears
        dqkv3, dqkv4 = torch.empty_like(qkv3), torch.empty_like(qkv4)
        attention_bwd(qkv3, qkv3, dy1, mx3, sm3, H, dqkv3, dqkv3, dr[SITE_SELF1])
        attention_bwd(qkv4, qkv4, dy2, mx4, sm4, H, dqkv4, dqkv4, dr[SITE_SELF2])
        dn3, _, _ = linear_bwd(dqkv3, n3, P["sa1"], dw=sink["sa1"])
        dn4, _, _ = linear_bwd(dqkv4, n4, P["sa2"], dw=sink["sa2"])
        # norm3 / norm4: d a (a residual gradient of xs2 / xs1 later) and its dropped copy for the proj linears
        da1, g1, _, _, _ = layernorm_bwd(dn3, a1, m3, r3, P["n3w"], drop=dr[SITE_PROJ1], dgamma=sink["n3w"], dbeta=sink["n3b"])
        da2, g2, _, _, _ = layernorm_bwd(dn4, a2, m4, r4, P["n4w"], drop=dr[SITE_PROJ2], dgamma=sink["n4w"], dbeta=sink["n4b"])
        do1, _, _ = linear_bwd(g1 if g1 is not None else da1, o1, P["p1w"], dw=sink["p1w"], db=sink["p1b"], has_bias=True)
        do2, _, _ = linear_bwd(g2 if g2 is not None else da2, o2, P["p2w"], dw=sink["p2w"], db=sink["p2b"], has_bias=True)
        # the two cross-attentions: each qkv buffer gets dq from its own attention and dk, dv from the other one
        dqkv1, dqkv2 = torch.empty_like(qkv1), torch.empty_like(qkv2)
        attention_bwd(qkv1, qkv2, do1, mx1, sm1, H, dqkv1, dqkv2, dr[SITE_ATTN1])
        attention_bwd(qkv2, qkv1, do2, mx2, sm2, H, dqkv2, dqkv1, dr[SITE_ATTN2])
        dn1x2, _, _ = linear_bwd(dqkv1, n1x2, P["qkv1"], dw=sink["qkv1"])
        dn2x1, _, _ = linear_bwd(dqkv2, n2x1, P["qkv2"], dw=sink["qkv2"])
        # norm1 reads xs2, norm2 reads xs1; xs2 also feeds a1 and y2, xs1 feeds a2 and y1
        dx2, _, _, _, _ = layernorm_bwd(dn1x2, xs2, m1, r1, P["n1w"], dy2, da1, npos=N, dgamma=sink["n1w"], dbeta=sink["n1b"],
                                        dpos=sink["pos2"])
        dx1, _, _, _, _ = layernorm_bwd(dn2x1, xs1, m2, r2, P["n2w"], dy1, da2, npos=N, dgamma=sink["n2w"], dbeta=sink["n2b"],
                                        dpos=sink["pos1"])
        for k in FUSION_PARAMS:
            if ret[k] is None:
                _grad_done(prm[k])
        as5 = lambda g: g.view(B, *ctx.sp[2:], C).permute(0, 4, 1, 2, 3)
        return (as5(dx1), as5(dx2), None, None, None, None, None, None) + tuple(ret[k] for k in FUSION_PARAMS)


def set_conv_engine(mode):
    """'auto' (MFMA implicit GEMM when the shape allows) or 'scalar' (gather kernels only; cross-check)."""
    call("mvd_set_conv_engine", {"auto": 0, "scalar": 1}[mode])


def lib_available():
    try:
        _lib.load()
        return True
    except (RuntimeError, OSError, AttributeError):
        return False
