"""Device-resident plan API (hmmsort_plan_* in include/hmmsort.h) for hosts that keep the signal
in HBM: bench.py and the multi-GPU driver.  Buffers are plain device pointers; torch is used only
as the allocator/stream provider (tensor.data_ptr(), torch.cuda.current_stream().cuda_stream)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import TRANS_DTYPE, check, lib, ptr


def _dptr(t):
    """device pointer of a torch tensor (or an int that already is one)."""
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    return C.c_void_p(t.data_ptr())


def stats_sum(d_parts, nparts, length, d_out, stream=0):
    """d_out[i] = sum over p of d_parts[p][i], p ascending, for `nparts` contiguous device vectors of `length`
    doubles (hmmsort_stats_sum): the fixed-order, on-device alternative to an all-reduce of statistics vectors."""
    check(lib().hmmsort_stats_sum(_dptr(d_parts), int(nparts), int(length), _dptr(d_out), C.c_void_p(stream)))


def stats_blend(d_acc, w, d_new, length, plain_tail=3, stream=0):
    """d_acc[i] = w * d_acc[i] + d_new[i] in two rounded steps for i < length - plain_tail, d_acc[i] += d_new[i] for
    the last `plain_tail` entries (hmmsort_stats_blend): exponentially weighted statistics, in place on the device.
    plain_tail = 3 is a path-statistics vector's x0, bad0, bad1."""
    check(lib().hmmsort_stats_blend(_dptr(d_acc), float(w), _dptr(d_new), int(length), int(plain_tail),
                                    C.c_void_p(stream)))


def seed_templates(d_y, N=3, K=60, resolve_overlaps=False, stream=None, **opts):
    """api.seed_templates for a float64 signal that is already resident (hmmsort_seed_templates_device): same options
    and the same (StateMatrix, mu, sigma, info), nothing but the results crosses to the host.  `stream`: a raw HIP
    stream handle, default torch's current one; the call synchronises it."""
    from .api import _seed_run
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    if not (d_y.is_floating_point() and d_y.element_size() == 8 and d_y.is_contiguous() and d_y.dim() == 1):
        raise TypeError("seed_templates: d_y must be a contiguous one-dimensional float64 device tensor")
    T = int(d_y.numel())
    return _seed_run(lambda opt, out: lib().hmmsort_seed_templates_device(_dptr(d_y), T, int(N), int(K), opt, out,
                                                                         C.c_void_p(stream)),
                     T, N, K, resolve_overlaps, opts)


def preprocess(d_raw, layout, taps=None, reference=None, groups=None, stream=None):
    """api.preprocess for a raw block that is already resident (hmmsort_preprocess_device): d_raw is a contiguous
    int16, int32, float32 or float64 device tensor of shape (T, C) with layout LAYOUT_SAMPLE_MAJOR or (C, T) with
    LAYOUT_CHANNEL_MAJOR (1-D: one channel).  Returns the [C][T] float64 tensor the batched plans take; the taps and
    groups are host arrays.  `stream`: a raw HIP stream handle, default torch's current one; the call synchronises
    it."""
    import torch
    from ._lib import LAYOUT_CHANNEL_MAJOR, LAYOUT_SAMPLE_MAJOR, SAMPLES_F32, SAMPLES_F64, SAMPLES_I16, SAMPLES_I32
    from .api import _pre_opt
    types = {torch.int16: SAMPLES_I16, torch.int32: SAMPLES_I32, torch.float32: SAMPLES_F32,
             torch.float64: SAMPLES_F64}
    if d_raw.dtype not in types or not d_raw.is_contiguous() or d_raw.dim() not in (1, 2):
        raise TypeError("preprocess: d_raw must be a contiguous 1-D or 2-D int16, int32, float32 or float64 device "
                        "tensor")
    if layout not in (LAYOUT_CHANNEL_MAJOR, LAYOUT_SAMPLE_MAJOR):
        raise ValueError("preprocess: unknown layout %r" % (layout,))
    if d_raw.dim() == 1:
        nC, T = 1, int(d_raw.numel())
    elif layout == LAYOUT_SAMPLE_MAJOR:
        T, nC = (int(n) for n in d_raw.shape)
    else:
        nC, T = (int(n) for n in d_raw.shape)
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    opt, alive = _pre_opt(taps, reference, groups, None)
    if alive[1] is not None and len(alive[1]) != nC:
        raise ValueError("preprocess: groups has %d entries for %d channels" % (len(alive[1]), nC))
    d_out = torch.empty((nC, T), dtype=torch.float64, device=d_raw.device)
    check(lib().hmmsort_preprocess_device(_dptr(d_raw), types[d_raw.dtype], int(layout), nC, T, C.byref(opt),
                                          _dptr(d_out), C.c_void_p(stream)))
    return d_out


def _f64_block(d_block, who):
    """(C, T) of a resident float64 block [C][T] (1-D: one channel)"""
    if not (d_block.is_floating_point() and d_block.element_size() == 8 and d_block.is_contiguous()
            and d_block.dim() in (1, 2)):
        raise TypeError("%s: the block must be a contiguous float64 device tensor of shape (C, T)" % who)
    return (1, int(d_block.numel())) if d_block.dim() == 1 else tuple(int(n) for n in d_block.shape)


def _stream(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    return C.c_void_p(stream)


def noise_scale(d_block, stream=None):
    """sigma per channel of a resident block [C][T]: the lower median of |y| over 0.6744897501960817, exact
    (hmmsort_noise_scale_device).  The call synchronises the stream."""
    nC, T = _f64_block(d_block, "noise_scale")
    sigma = np.zeros(nC)
    check(lib().hmmsort_noise_scale_device(_dptr(d_block), nC, T, ptr(sigma), _stream(stream)))
    return sigma


def noise_covariance(d_block, threshold=4.0, guard=30, thr=None, d_quiet=None, stream=None):
    """api.noise_sums for a block that is already resident (hmmsort_noise_cov_device): (sigma or None, thr, n_quiet, s1,
    s2); only these cross to the host.  d_quiet: an optional uint8 device tensor of T entries that receives the quiet
    mask.  `stream`: a raw HIP stream handle, default torch's current one; the call synchronises it."""
    from .api import _noise_args, _noise_result
    nC, T = _f64_block(d_block, "noise_covariance")
    opt, out, alive = _noise_args(nC, threshold, guard, thr)
    if d_quiet is not None:
        if d_quiet.element_size() != 1 or not d_quiet.is_contiguous() or int(d_quiet.numel()) != T:
            raise TypeError("noise_covariance: d_quiet must be a contiguous uint8 device tensor of T = %d entries" % T)
        out.d_quiet = d_quiet.data_ptr()
    check(lib().hmmsort_noise_cov_device(_dptr(d_block), nC, T, C.byref(opt), C.byref(out), _stream(stream)))
    return _noise_result(opt, alive)


def channel_mix(d_in, nbr, w, d_out=None, stream=None):
    """api.channel_mix for a resident block [C][T] (hmmsort_channel_mix_device): nbr and w are host arrays (R, M).
    d_out: the (R, T) float64 tensor to write, default a new one; d_out = d_in mixes in place (R == C), and no second
    block exists.  Returns d_out.  The call synchronises the stream."""
    import torch
    from .api import _mix_args
    nC, T = _f64_block(d_in, "channel_mix")
    nbr, w = _mix_args(nbr, w, "channel_mix")
    R, M = nbr.shape
    if d_out is None:
        d_out = torch.empty((R, T), dtype=torch.float64, device=d_in.device)
    elif _f64_block(d_out, "channel_mix") != (R, T):
        raise ValueError("channel_mix: d_out must be (%d, %d), got %s" % (R, T, tuple(d_out.shape)))
    check(lib().hmmsort_channel_mix_device(_dptr(d_in), nC, T, R, M, ptr(nbr), ptr(w), _dptr(d_out), _stream(stream)))
    return d_out


def whiten(d_block, threshold=4.0, guard=30, thr=None, neighbors=None, eps_rel=1e-6, whitening=None, inplace=False,
           stream=None):
    """api.whiten on a resident block [C][T]: noise scale, quiet mask and sums on the device, api.noise_covariance and
    api.whitening_matrix on the host (C x C numbers), the mix on the device.  Returns (d_out, api.Whitening);
    inplace=True writes the block itself, and no second [C][T] buffer exists.  A given `whitening` is applied as it
    is."""
    from . import api
    wh = whitening
    if wh is None:
        sigma, th, n, s1, s2 = noise_covariance(d_block, threshold, guard, thr, stream=stream)
        cov = api.noise_covariance(n, s1, s2)
        nbr, w = api.whitening_matrix(cov, neighbors, eps_rel)
        wh = api.Whitening(sigma, th, 30 if guard is None or guard < 0 else int(guard), n, s1, s2, cov, nbr, w)
    d2 = d_block if d_block.dim() == 2 else d_block[None, :]
    return channel_mix(d2, wh.nbr, wh.w, d2 if inplace else None, stream), wh


def _fp_block(d_block):
    """(C, T) of a resident float64 block [C][T] (1-D: one channel)"""
    if not (d_block.is_floating_point() and d_block.element_size() == 8 and d_block.is_contiguous()
            and d_block.dim() in (1, 2)):
        raise TypeError("footprints: the block must be a contiguous float64 device tensor of shape (C, T)")
    return (1, int(d_block.numel())) if d_block.dim() == 1 else tuple(int(n) for n in d_block.shape)


def footprints(d_block, d_times, offs, pre=20, W=60, channels=None, stream=None):
    """api.footprints for a block and spike lists that are already resident (hmmsort_footprints_device): d_block the
    [C][T] float64 tensor (device.preprocess's output), d_times one int64 device tensor holding the U lists one after
    the other (1-based samples, each list ascending), offs the U + 1 host offsets into it.  Returns api.Footprints;
    only the sums cross to the host.  `stream`: a raw HIP stream handle, default torch's current one; the call
    synchronises it."""
    from .api import _fp_run
    nC, T = _fp_block(d_block)
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    offs = np.ascontiguousarray(offs, dtype=np.int64).ravel()
    U = len(offs) - 1
    if d_times.element_size() != 8 or d_times.is_floating_point() or not d_times.is_contiguous():
        raise TypeError("footprints: d_times must be a contiguous int64 device tensor")
    if U >= 1 and int(offs[-1]) > int(d_times.numel()):
        raise ValueError("footprints: offs ends at %d, d_times has %d entries" % (offs[-1], d_times.numel()))
    return _fp_run(lambda opt, out: lib().hmmsort_footprints_device(_dptr(d_block), nC, T, U, _dptr(d_times),
                                                                    ptr(offs), opt, out, C.c_void_p(stream)),
                   U, nC, pre, W, channels)


def _feat_device_run(call, U, nC, n_total, pre, W, channels, basis, centre, moments, features, like):
    """call(byref(opt), byref(out)) -> rc with device rows: the SnippetFeatures of a device or plan features call.
    n_total None: the plan form, which learns the rows from a first call without them"""
    import torch
    from .api import SnippetFeatures, _feat_args
    opt, out, arr, (M, P, F) = _feat_args(U, nC, pre, W, channels, basis, centre, moments)
    if n_total is None and features:
        first = _lib.FeatOpt(opt.pre, opt.W, opt.M, opt.chan, opt.P, opt.basis, opt.centre, 0)
        check(call(C.byref(first), C.byref(out)))
        n_total = int(arr["n"].sum())
    d_feat = d_used = None
    if features and n_total * F <= 1 << 31:
        d_feat = torch.zeros((n_total, F), dtype=torch.float64, device=like.device)
        d_used = torch.zeros(n_total, dtype=torch.uint8, device=like.device)
        out.feat, out.used, out.cap_rows = d_feat.data_ptr() or None, d_used.data_ptr() or None, n_total
    elif features:
        out.feat, out.cap_rows = like.data_ptr(), 0    # the library refuses the size before it looks at the pointer
    check(call(C.byref(opt), C.byref(out)))
    return SnippetFeatures(d_feat, d_used, arr["n"], arr["nused"], arr.get("b1"), arr.get("b2"), arr.get("g1"),
                           arr.get("g2"))


def snippet_features(d_block, d_times, offs, pre=20, W=60, channels=None, basis=None, centre=None, moments=0,
                     features=True, stream=None):
    """api.snippet_features for a block and spike lists that are already resident (hmmsort_snippet_features_device;
    arguments as device.footprints, `channels` one list for all units).  The rows and the used bytes stay on the
    device (torch tensors of the result); the counts and moments come to the host.  Synchronises `stream`."""
    nC, T = _fp_block(d_block)
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    offs = np.ascontiguousarray(offs, dtype=np.int64).ravel()
    U = len(offs) - 1
    if d_times.element_size() != 8 or d_times.is_floating_point() or not d_times.is_contiguous():
        raise TypeError("snippet_features: d_times must be a contiguous int64 device tensor")
    if U >= 1 and int(offs[-1]) > int(d_times.numel()):
        raise ValueError("snippet_features: offs ends at %d, d_times has %d entries" % (offs[-1], d_times.numel()))
    n_total = max(0, int(offs[-1] - offs[0])) if U >= 1 else 0
    return _feat_device_run(lambda opt, out: lib().hmmsort_snippet_features_device(
        _dptr(d_block), nC, T, U, _dptr(d_times), ptr(offs), opt, out, C.c_void_p(stream)),
        U, nC, n_total, pre, W, channels, basis, centre, moments, features, d_block)


def isolation_scores(d_feat, offs, mu, Vinv, d_used=None, stream=None):
    """api.isolation_scores on resident rows (hmmsort_cluster_isolation_device): d_feat [n][F] float64 and d_used [n]
    uint8 device tensors (d_used None: every row used).  Returns (iso_d2, closer, lpair) on the host."""
    from .api import _iso_run
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    if not (d_feat.dim() == 2 and d_feat.is_contiguous() and d_feat.is_floating_point() and d_feat.element_size() == 8):
        raise TypeError("isolation_scores: d_feat must be a contiguous float64 device tensor [n][F]")
    n, F = (int(v) for v in d_feat.shape)
    offs = np.ascontiguousarray(offs, dtype=np.int64).ravel()
    U = len(offs) - 1
    mu, Vinv = np.ascontiguousarray(mu, dtype=np.float64), np.ascontiguousarray(Vinv, dtype=np.float64)
    if mu.shape != (U, F) or Vinv.shape != (U, F, F):
        raise ValueError("isolation_scores: mu must be [%d][%d] and Vinv [%d][%d][%d]" % (U, F, U, F, F))
    if d_used is not None and (d_used.element_size() != 1 or not d_used.is_contiguous() or d_used.numel() != n):
        raise TypeError("isolation_scores: d_used must be a contiguous uint8 device tensor of %d entries" % n)
    return _iso_run(lambda out: lib().hmmsort_cluster_isolation_device(
        _dptr(d_feat), n, F, U, ptr(offs), None if d_used is None else _dptr(d_used), ptr(mu), ptr(Vinv), out,
        C.c_void_p(stream)), U)


def _isolation_from(run, P, keep_features):
    """the two passes of api.cluster_isolation over run(basis, centre, moments, features) -> SnippetFeatures with
    device rows"""
    from . import api
    p1 = run(None, None, 1, False)
    basis, centre = api.pca_basis(p1.b1, p1.b2, p1.n_used, P)
    p2 = run(basis, centre, 2, True)
    mu, vinv = api.unit_gaussians(p2.g1, p2.g2, p2.n_used)
    d2, closer, lpair = isolation_scores(p2.features, p2.offs, mu, vinv, p2.used)
    return api._isolation_result(d2, closer, lpair, p2.n_used, basis, centre, p2.features if keep_features else None)


def cluster_isolation(d_block, d_times, offs, pre=20, W=60, channels=None, P=3, keep_features=False, stream=None):
    """api.cluster_isolation for a resident block and resident lists: both feature passes, the distances, the order
    statistic and the sums on the device, the rows never leave it (keep_features=True returns them as a device
    tensor); the PCA and the F x F inverses on the host."""
    return _isolation_from(lambda basis, centre, moments, features: snippet_features(
        d_block, d_times, offs, pre, W, channels, basis, centre, moments, features, stream), P, keep_features)


def unit_stability(d_times, offs, d_values=None, T=None, bin=None, quantiles=(1 / 4, 1 / 2, 3 / 4), hist=None,
                   stream=None):
    """api.unit_stability for spike lists and values that are already resident (hmmsort_unit_stability_device):
    d_times one int64 device tensor holding the U lists one after the other, d_values a float64 device tensor laid out
    the same way (None: counts only), offs the U + 1 host offsets.  Returns api.UnitStability; only the tables cross to
    the host.  The call synchronises `stream` (default torch's current one)."""
    from .api import _stab_run
    if T is None or bin is None:
        raise ValueError("unit_stability: T and bin are required")
    offs = np.ascontiguousarray(offs, dtype=np.int64).ravel()
    U = len(offs) - 1
    if d_times.element_size() != 8 or d_times.is_floating_point() or not d_times.is_contiguous():
        raise TypeError("unit_stability: d_times must be a contiguous int64 device tensor")
    if d_values is not None and not (d_values.is_floating_point() and d_values.element_size() == 8
                                     and d_values.is_contiguous()):
        raise TypeError("unit_stability: d_values must be a contiguous float64 device tensor")
    for name, t in (("d_times", d_times), ("d_values", d_values)):
        if t is not None and U >= 1 and int(offs[-1]) > int(t.numel()):
            raise ValueError("unit_stability: offs ends at %d, %s has %d entries" % (offs[-1], name, t.numel()))
    return _stab_run(lambda opt, out: lib().hmmsort_unit_stability_device(
        U, _dptr(d_times), _dptr(d_values), ptr(offs), opt, out, _stream(stream)), U, T, bin, quantiles, hist,
        d_values is not None)


class Plan:
    """One recording channel of length T with a fixed model shape."""

    def __init__(self, T, lA, mu, sigma):
        self._h = C.c_void_p(None)
        self.T = int(T)
        self.lA = lA
        mu = np.asfortranarray(mu, dtype=np.float64)
        tr = np.ascontiguousarray(lA.transitions, dtype=TRANS_DTYPE)
        st = np.asfortranarray(lA.states, dtype=np.int16)
        check(lib().hmmsort_plan_create(C.byref(self._h), self.T, ptr(st), lA.N, lA.K, lA.nstates,
                                        ptr(tr), len(tr), ptr(mu), float(sigma)))
        self.K, self.N, self.S = lA.K, lA.N, lA.nstates

    @classmethod
    def batched(cls, T, lAs, mus, sigmas):
        """C channels of length T with per-channel models of one shape (hmmsort_plan_create_batched).
        Device buffers of every call are channel-major: y [C][T], x [C][T], ll [C], stats [C][len]."""
        self = cls.__new__(cls)
        self._h = C.c_void_p(None)
        self.T = int(T)
        lA = lAs[0]
        self.lA = lA
        nC = len(lAs)
        R = len(lA.transitions)
        tr = np.ascontiguousarray(np.stack([np.ascontiguousarray(a.transitions, dtype=TRANS_DTYPE) for a in lAs]))
        assert tr.shape == (nC, R), "batched plan: every channel needs the same transition count"
        mu = np.ascontiguousarray(np.stack([np.asfortranarray(m, dtype=np.float64).ravel(order="F") for m in mus]))
        sg = np.ascontiguousarray(sigmas, dtype=np.float64)
        st = np.asfortranarray(lA.states, dtype=np.int16)
        check(lib().hmmsort_plan_create_batched(C.byref(self._h), nC, self.T, ptr(st), lA.N, lA.K, lA.nstates,
                                                ptr(tr), R, ptr(mu), ptr(sg)))
        self.K, self.N, self.S = lA.K, lA.N, lA.nstates
        self.C = nC
        return self

    def channels(self):
        return int(lib().hmmsort_plan_channels(self._h))

    def set_model_channel(self, ch, lA, mu, sigma):
        mu = np.asfortranarray(mu, dtype=np.float64)
        tr = np.ascontiguousarray(lA.transitions, dtype=TRANS_DTYPE)
        check(lib().hmmsort_plan_set_model_channel(self._h, int(ch), ptr(tr), len(tr), ptr(mu), float(sigma)))

    def close(self):
        if self._h:
            lib().hmmsort_plan_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def info(self):
        v = [C.c_int64(0) for _ in range(5)]
        check(lib().hmmsort_plan_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("engine", "block", "halo", "nchains", "workspace_bytes"),
                        [x.value for x in v]))

    def overlap_sweep(self):
        """which sweep an overlap model runs on the blocked engine: 0 generic, 2 pair sweep, 3..5 multi sweep"""
        return int(lib().hmmsort_plan_overlap_sweep(self._h))

    def set_model(self, lA, mu, sigma):
        mu = np.asfortranarray(mu, dtype=np.float64)
        tr = np.ascontiguousarray(lA.transitions, dtype=TRANS_DTYPE)
        check(lib().hmmsort_plan_set_model(self._h, ptr(tr), len(tr), ptr(mu), float(sigma)))
        self.lA = lA

    def bind(self, d_y, stream=0):
        """transpose + ring-score pre-pass once; following viterbi/estep calls on d_y reuse them"""
        check(lib().hmmsort_plan_bind(self._h, _dptr(d_y), C.c_void_p(stream)))

    def unbind(self):
        check(lib().hmmsort_plan_unbind(self._h))

    def viterbi(self, d_y, d_x, d_ll, stream=0):
        check(lib().hmmsort_plan_viterbi(self._h, _dptr(d_y), _dptr(d_x), _dptr(d_ll),
                                         C.c_void_p(stream)))

    def set_shard(self, own_lo, own_hi, first, last):
        """time shard of a longer recording: accumulate statistics for [own_lo, own_hi) only"""
        check(lib().hmmsort_plan_set_shard(self._h, int(own_lo), int(own_hi), int(bool(first)),
                                           int(bool(last))))

    def stats_len(self):
        return int(lib().hmmsort_plan_stats_len(self._h))

    def mstep_len(self):
        """doubles per channel of the M-step output [mu (K x N) | sigma | xb[2:end] | pp (S)], as the library
        writes them (hmmsort_plan_mstep_len): N entry log-probabilities for wave/ring plans whatever the
        list has dropped (types.jl:121), one per transition leaving state 1 but the first otherwise
        (baumwelch.jl:226,264)"""
        return int(lib().hmmsort_plan_mstep_len(self._h))

    def estep(self, d_y, d_stats, stream=0):
        check(lib().hmmsort_plan_estep(self._h, _dptr(d_y), _dptr(d_stats), C.c_void_p(stream)))

    def decode_estep(self, d_y, d_x, d_ll, d_stats, stream=0):
        """viterbi + estep of the same signal/model with the three sweeps sharing one launch"""
        check(lib().hmmsort_plan_decode_estep(self._h, _dptr(d_y), _dptr(d_x), _dptr(d_ll),
                                              _dptr(d_stats), C.c_void_p(stream)))

    def mstep(self, d_stats, d_out, stream=0):
        check(lib().hmmsort_plan_mstep(self._h, _dptr(d_stats), _dptr(d_out), C.c_void_p(stream)))

    def path_update(self, d_y, d_x, out, counts=None, stream=0):
        """Viterbi training: the model re-estimated from the path d_x of d_y (hmmsort_plan_path_update), device to
        device.  `out`: mstep_len() doubles per channel in mstep's layout; `counts`: three int64 per channel
        (ids outside 1..S, pairs that are no transition of the list, template rows that kept their mean) or None."""
        check(lib().hmmsort_plan_path_update(self._h, _dptr(d_y), _dptr(d_x), _dptr(out), _dptr(counts),
                                             C.c_void_p(stream)))

    def path_stats_len(self):
        """doubles per channel of the path statistics: 3 N (K-1) + S + n_lp + 6 (hmmsort_plan_path_stats_len)"""
        return int(lib().hmmsort_plan_path_stats_len(self._h))

    def path_stats(self, d_y, d_x, T, own_lo, own_hi, first, d_stats, stream=0):
        """Additive statistics of Viterbi training over samples [own_lo, own_hi) of the arrays d_y / d_x of length
        T (hmmsort_plan_path_stats).  T is the arrays' length, not the plan's: a plan of chunk length serves a
        whole recording.  The vectors of shards, chunks or channels add (all-reduce, stats_sum); path_finish
        turns the sum into the new model."""
        check(lib().hmmsort_plan_path_stats(self._h, _dptr(d_y), _dptr(d_x), int(T), int(own_lo), int(own_hi),
                                            int(bool(first)), _dptr(d_stats), C.c_void_p(stream)))

    def path_finish(self, d_stats, out, counts=None, stream=0):
        """path statistics and the plan's current model -> `out` and `counts` as path_update writes them
        (hmmsort_plan_path_finish)"""
        check(lib().hmmsort_plan_path_finish(self._h, _dptr(d_stats), _dptr(out), _dptr(counts),
                                             C.c_void_p(stream)))

    def diagnostics(self, stream=0):
        d = (C.c_int64 * 8)()
        check(lib().hmmsort_plan_diagnostics(self._h, C.c_void_p(stream), d))
        out = list(d)
        import struct
        for i in (2, 4, 6):  # largest boundary errors travel as double bit patterns
            out[i] = struct.unpack("<d", struct.pack("<q", out[i]))[0]
        return out

    def tie_stats(self, stream=0):
        """what the exact near-tie resolver did in the last decode (hmmsort_plan_tie_stats)"""
        d = (C.c_int64 * 8)()
        check(lib().hmmsort_plan_tie_stats(self._h, C.c_void_p(stream), d))
        return dict(zip(("trigger", "flagged", "decided", "flips", "unresolved", "tail", "longest_walk",
                         "serial_blocks"), list(d)))

    def reconstruct(self, d_x, d_y_out, stream=0):
        """reconstruct_signal of a decoded path, device to device (T doubles)"""
        check(lib().hmmsort_plan_reconstruct(self._h, _dptr(d_x), _dptr(d_y_out), C.c_void_p(stream)))

    def unroll_mlseq(self, d_x, d_out, stream=0):
        """unroll_mlseq of a decoded path, device to device (N x T int16, column-major)"""
        check(lib().hmmsort_plan_unroll_mlseq(self._h, _dptr(d_x), _dptr(d_out), C.c_void_p(stream)))

    def extract_spiketimes(self, d_x, stream=0):
        """extract_spiketimes (extraction.jl:15-24) from the decoded path in device memory:
        list of 1-based sample-index arrays, one per neuron (only the spike times leave the GPU)."""
        counts = np.zeros(self.N, dtype=np.int64)
        check(lib().hmmsort_plan_extract_spiketimes(self._h, _dptr(d_x), None, 0, ptr(counts),
                                                    C.c_void_p(stream)))
        cap = int(counts.max()) if self.N else 0
        times = np.zeros((self.N, max(cap, 1)), dtype=np.int64)
        if cap:
            check(lib().hmmsort_plan_extract_spiketimes(self._h, _dptr(d_x), ptr(times), cap,
                                                        ptr(counts), C.c_void_p(stream)))
        return [times[i, :counts[i]].copy() for i in range(self.N)]

    def posteriors(self, d_y, d_onset=None, d_occ=None, d_silent=None, d_logz=None, stream=0):
        """smoothed state posteriors of d_y under the plan's model, device to device (hmmsort_plan_posteriors):
        onset / occ [C][N][T], silent [C][T], logz [C] doubles; None skips an output.  Wave plans (ring models),
        blocked plans (overlap models within the blocked E-step's LDS limit, up to 4 templates; asynchronous,
        no S x T workspace) and strict plans (any model, 2 x S x T doubles); the plan keeps the posteriors for
        posterior_decode / spike_confidence / expected_counts until its next E-step, set_model or posterior
        call."""
        check(lib().hmmsort_plan_posteriors(self._h, _dptr(d_y), _dptr(d_onset), _dptr(d_occ), _dptr(d_silent),
                                            _dptr(d_logz), C.c_void_p(stream)))

    def posterior_decode(self, d_xm, stream=0):
        """arg max_s gamma_t(s) per sample ([C][T] int16, 1-based states), after posteriors()"""
        check(lib().hmmsort_plan_posterior_decode(self._h, _dptr(d_xm), C.c_void_p(stream)))

    def spike_confidence(self, d_x, jitter=2, stream=0):
        """per template (times, confidence) of the events extract_spiketimes reports on the decoded path d_x,
        after posteriors(): confidence = posterior probability that the template was in its trough state within
        +-jitter samples of the event.  A batched plan returns one such list per channel."""
        nC = getattr(self, "C", 1)
        counts = np.zeros((nC, self.N), dtype=np.int64)
        check(lib().hmmsort_plan_spike_confidence(self._h, _dptr(d_x), int(jitter), None, None, 0, ptr(counts),
                                                  C.c_void_p(stream)))
        cap = max(int(counts.max()) if counts.size else 0, 1)
        times = np.zeros((nC, self.N, cap), dtype=np.int64)
        conf = np.zeros((nC, self.N, cap), dtype=np.float64)
        check(lib().hmmsort_plan_spike_confidence(self._h, _dptr(d_x), int(jitter), ptr(times), ptr(conf), cap,
                                                  ptr(counts), C.c_void_p(stream)))
        out = [[(times[c, i, :counts[c, i]].copy(), conf[c, i, :counts[c, i]].copy()) for i in range(self.N)]
               for c in range(nC)]
        return out if hasattr(self, "C") else out[0]

    def spike_fit(self, d_y, d_x, track=None, stream=0):
        """per template an api.SpikeFit of the events extract_spiketimes reports on the path d_x of the resident
        signal d_y, under the plan's current model (hmmsort_plan_spike_fit): amplitude, residual at unit amplitude,
        energy and used phases per spike, and the per-template summary.  `track`: fit_adaptive's ModelTrack
        (single-channel plans only).  A batched plan returns one such list per channel."""
        from .api import _spike_fit_run, _track_args
        nC = getattr(self, "C", 1)
        nch, first, mut = _track_args(self.lA, track)
        out = _spike_fit_run(lambda o: lib().hmmsort_plan_spike_fit(self._h, _dptr(d_y), _dptr(d_x), nch, ptr(first),
                                                                    ptr(mut), o, C.c_void_p(stream)),
                             nC, self.N, self.K, max(1, self.T // 8))
        return out if hasattr(self, "C") else out[0]

    def correlograms(self, d_x, bin=30, half_bins=50, refractory=30, coincidence=2, stream=0):
        """api.Correlograms of the events extract_spiketimes reports on the resident path(s) d_x under the plan's
        current model (hmmsort_plan_correlograms): units are u = channel * N + template, pairs across the channels
        of a batched plan included.  The events are compacted on the device and stay there; only the counts cross."""
        from .api import _ccg_run
        U = getattr(self, "C", 1) * self.N
        return _ccg_run(lambda opt, out: lib().hmmsort_plan_correlograms(self._h, _dptr(d_x), opt, out,
                                                                         C.c_void_p(stream)),
                        U, bin, half_bins, refractory, coincidence)

    def footprints(self, d_x, d_block, pre=20, W=60, channels=None, stream=0):
        """api.Footprints of the events extract_spiketimes reports on the resident path(s) d_x under the plan's current
        model, on every channel of the resident float64 block d_block [Cb][T] of the plan's T (hmmsort_plan_footprints):
        units are u = channel * N + template.  Cb need not be the plan's channel count: a one-channel plan can be
        measured against the whole block its channel came from.  The events are compacted on the device and stay
        there; only the sums cross."""
        from .api import _fp_run
        nC, T = _fp_block(d_block)
        if T != self.T:
            raise ValueError("footprints: the block has %d samples per channel, the plan %d" % (T, self.T))
        U = getattr(self, "C", 1) * self.N
        return _fp_run(lambda opt, out: lib().hmmsort_plan_footprints(self._h, _dptr(d_x), _dptr(d_block), nC, opt, out,
                                                                      C.c_void_p(stream)),
                       U, nC, pre, W, channels)

    def snippet_features(self, d_x, d_block, pre=20, W=60, channels=None, basis=None, centre=None, moments=0,
                         features=True, stream=0):
        """api.SnippetFeatures of the events extract_spiketimes reports on the resident path(s) d_x under the plan's
        current model, on the resident float64 block d_block [Cb][T] (hmmsort_plan_snippet_features): units are
        u = channel * N + template, rows in that order.  With features=True a first call learns the counts, then the
        rows are written to device tensors of exactly that size; the events themselves never come to the host."""
        nC, T = _fp_block(d_block)
        if T != self.T:
            raise ValueError("snippet_features: the block has %d samples per channel, the plan %d" % (T, self.T))
        U = getattr(self, "C", 1) * self.N
        return _feat_device_run(lambda opt, out: lib().hmmsort_plan_snippet_features(
            self._h, _dptr(d_x), _dptr(d_block), nC, opt, out, C.c_void_p(stream)),
            U, nC, None, pre, W, channels, basis, centre, moments, features, d_block)

    def cluster_isolation(self, d_x, d_block, pre=20, W=60, channels=None, P=3, keep_features=False, stream=0):
        """api.Isolation of the plan's units on the resident block: device.cluster_isolation on the plan form."""
        return _isolation_from(lambda basis, centre, moments, features: self.snippet_features(
            d_x, d_block, pre, W, channels, basis, centre, moments, features, stream), P, keep_features)

    def unit_stability(self, d_y, d_x, bin, quantiles=(1 / 4, 1 / 2, 3 / 4), hist=None, stream=0):
        """api.UnitStability of the events extract_spiketimes reports on the resident path(s) d_x of the resident
        signal(s) d_y under the plan's current model, with spike_fit's amplitude as the value of every event
        (hmmsort_plan_unit_stability): units are u = channel * N + template.  Events and amplitudes stay on the
        device; only the tables cross."""
        from .api import _stab_run
        U = getattr(self, "C", 1) * self.N
        return _stab_run(lambda opt, out: lib().hmmsort_plan_unit_stability(self._h, _dptr(d_y), _dptr(d_x), opt, out,
                                                                            C.c_void_p(stream)),
                         U, self.T, bin, quantiles, hist, True)

    def expected_counts(self, stream=0):
        """expected number of spikes per template, sum_t onset[a, t] ([C][N]; [N] for a single-channel plan)"""
        nC = getattr(self, "C", 1)
        out = np.zeros((nC, self.N), dtype=np.float64)
        check(lib().hmmsort_plan_expected_counts(self._h, ptr(out), C.c_void_p(stream)))
        return out if hasattr(self, "C") else out[0]

    def profile(self, enable=True):
        check(lib().hmmsort_plan_profile(self._h, int(bool(enable))))

    def profile_read(self, stream=0):
        """{kernel name: (total ms, launches)} since the previous read (synchronises the stream)."""
        cap = 64
        names = C.create_string_buffer(4096)
        ms = (C.c_double * cap)()
        calls = (C.c_int64 * cap)()
        n = C.c_int64(0)
        check(lib().hmmsort_plan_profile_read(self._h, C.c_void_p(stream), names, 4096, ms, calls,
                                              cap, C.byref(n)))
        nm = names.value.decode().split("\n") if n.value else []
        return {nm[i]: (ms[i], calls[i]) for i in range(n.value)}
