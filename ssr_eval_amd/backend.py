"""Host-side plumbing between the reference-shaped Python API and libssrhip.so.

PyTorch-ROCm is used for device memory, streams and (in ``ssr_eval_amd.dist``) RCCL; every number is
produced by the HIP kernels behind the C ABI.  Batches are ragged: one flat float32 device buffer plus
int64 offsets / int32 lengths, all resident in HBM.
"""
import ctypes as C
import os
import math
import threading

import numpy as np
import torch

from . import _lib
from ._lib import M_ALL, M_LOG_SISPEC, M_LSD, M_SISPEC, M_SSIM, SsrHipError  # noqa: F401

_PREC = {"f32": _lib.SSR_F32, "f64": _lib.SSR_F64, _lib.SSR_F32: _lib.SSR_F32, _lib.SSR_F64: _lib.SSR_F64}


def require_gpu():
    if not torch.cuda.is_available():
        raise SsrHipError("ssr_eval_amd needs a HIP device (torch.cuda.is_available() is False); there is no CPU path")


def default_device():
    require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_index(dev):
    """The index of a torch device (the current device's where it names none)."""
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _workspace(nbytes, dev):
    """The scratch buffer of one library call (never zero-sized: the library takes a non-null pointer)."""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def _offsets(lens):
    """Exclusive prefix sums (int64): where each item of a batch packed back to back starts."""
    lens = np.asarray(lens, dtype=np.int64)
    return np.cumsum(lens) - lens


def _uniform_images(N, T, dev):
    """(offsets int64 [N], lengths int32 [N]) of N items of T rows (or samples) each, built on the device."""
    return torch.arange(N, device=dev, dtype=torch.int64) * T, torch.full((N,), T, device=dev, dtype=torch.int32)


def num_frames(n, n_fft, hop):
    """T of a centred STFT (bit-exact integer)."""
    return 1 + (int(n) + 2 * (n_fft // 2) - n_fft) // hop


def _tl_dft_matrices(n):
    """torchlibrosa DFTBase.dft_matrix / idft_matrix (stft.py): W[x, y] = omega ** (x y) with omega = exp(-/+ 2 pi i / n), evaluated
    as the module evaluates it - numpy's complex128 power on the integer product grid - so that the float32 weights below are the
    reference's to the last bit (ssr_eval/dsp.py:21-39 builds STFT / ISTFT, which build these).  The power is a function of the
    exponent alone, so it is taken once per DISTINCT product x y (a quarter of the grid) and gathered: the same values, 3-4x sooner."""
    x, y = np.meshgrid(np.arange(n), np.arange(n))
    k, inv = np.unique(x * y, return_inverse=True)
    inv = inv.reshape(n, n)
    return np.power(np.exp(-2 * np.pi * 1j / n), k)[inv], np.power(np.exp(2 * np.pi * 1j / n), k)[inv]


def tl_conv_weights(n_fft, window=None):
    """The float32 Conv1d weights of torchlibrosa's STFT / ISTFT for a float64 window [n_fft] (None: periodic Hann =
    librosa.filters.get_window("hann", n_fft, fftbins=True)), in the modules' layout:
    (fwd_re, fwd_im [n_bins, n_fft]; inv_re, inv_im [n_fft (output sample), n_fft (channel)]; float32(window ** 2))."""
    n, F = int(n_fft), int(n_fft) // 2 + 1
    W, Wi = _tl_dft_matrices(n)
    if window is None:
        import scipy.signal
        window = scipy.signal.get_window("hann", n, fftbins=True)
    win = np.asarray(window, dtype=np.float64)
    fw = W[:, :F] * win[:, None]                      # STFT.__init__: conv weights = (W[:, 0:out_channels] * window[:, None]).T
    iw = (Wi / n) * win[None, :]                      # ISTFT.init_real_imag_conv: (W / n_fft * ifft_window[None, :]).T
    c32 = lambda a: np.ascontiguousarray(a).astype(np.float32)          # noqa: E731
    return (c32(np.real(fw).T), c32(np.imag(fw).T), c32(np.real(iw).T), c32(np.imag(iw).T), (win ** 2).astype(np.float32))


class Plan:
    """An immutable ssr_plan (window / twiddle / Bluestein tables in HBM) for one (n_fft, hop, precision)."""

    def __init__(self, n_fft, hop, precision="f64", device=None):
        require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device) if device is not None else default_device()
        self.n_fft, self.hop, self.n_bins = int(n_fft), int(hop), int(n_fft) // 2 + 1
        self.precision = _PREC[precision]
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ssr_plan_create(self.n_fft, self.hop, self.precision, C.byref(h)))
        self.handle = h
        q = [C.c_int() for _ in range(6)]
        _lib.check(self.lib.ssr_plan_query(h, *[C.byref(x) for x in q]))
        self.fft_len, self.bluestein = q[3].value, bool(q[4].value)

    def frames(self, n):
        return num_frames(n, self.n_fft, self.hop)

    def check_lengths(self, lens_host):
        """torch-style reflect padding (torchlibrosa STFT / ISTFT: F.pad refuses a pad >= the signal length)."""
        if len(lens_host) and int(np.min(lens_host)) <= self.n_fft // 2:
            raise ValueError("reflect padding needs every signal longer than n_fft//2 = %d samples" % (self.n_fft // 2))

    def set_lowpass_engine(self, engine):
        """"segments" (frame kernel + overlap-add kernel through the workspace), "fused" (one kernel, no workspace traffic;
        float64 2048-point plans with 228 <= hop <= 914) or "conv" (torchlibrosa's dense float32 DFT products on the matrix cores:
        the reference's arithmetic class).  See include/ssr_hip.h: ssr_plan_set_lowpass_engine.  A plan handed out by
        get_plan() is cached under its engine and refuses a change."""
        if getattr(self, "_cached", False) and engine != getattr(self, "lowpass_engine", "segments"):
            raise ValueError("this plan is shared through get_plan() under its engine; ask get_plan(..., lowpass_engine=%r)" % engine)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ssr_plan_set_lowpass_engine(self.handle, _ENGINES[engine]))
            if engine == "conv":
                self._upload_tl_weights(None)
        self.lowpass_engine = engine
        return self

    def _upload_tl_weights(self, window):
        """The conv engine multiplies by torchlibrosa's OWN weight values (tl_conv_weights: the module's numpy expressions), not by
        the library's independently computed tables (1 ulp apart in ~0.5 % of the entries)."""
        tabs = tl_conv_weights(self.n_fft, window)
        _lib.check(self.lib.ssr_plan_set_tl_weights(self.handle, *[t.ctypes.data_as(C.c_void_p) for t in tabs]))

    def __del__(self):
        try:
            if getattr(self, "handle", None) is not None and self.handle.value:
                self.lib.ssr_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class PlanEx(Plan):
    """ssr_plan_create_ex: FDomainHelper(center=, pad_mode=, window=) beyond the defaults (ssr_eval/dsp.py:7-59) - the conv engine
    with torchlibrosa's weights built from `window` (float64 [n_fft], librosa.filters.get_window(name, n_fft, fftbins=True); None =
    periodic Hann), no padding when center is False, zeros instead of the reflection for pad_mode "constant".  Serves stft(kind=
    "complex"), istft and LowpassBatch / lowpass only."""

    _PAD = {"reflect": _lib.PAD_REFLECT, "constant": _lib.PAD_CONSTANT}

    def __init__(self, n_fft, hop, window=None, center=True, pad_mode="reflect", device=None):
        require_gpu()
        if pad_mode not in self._PAD:
            raise NotImplementedError("pad_mode %r: torch's F.pad modes 'reflect' and 'constant' are implemented" % (pad_mode,))
        self.lib = _lib.load()
        self.device = torch.device(device) if device is not None else default_device()
        self.n_fft, self.hop, self.n_bins = int(n_fft), int(hop), int(n_fft) // 2 + 1
        self.precision = _PREC["f32"]
        self.center, self.pad_mode = bool(center), pad_mode
        w = None if window is None else np.ascontiguousarray(window, dtype=np.float64)
        if w is not None and w.shape != (self.n_fft,):
            raise ValueError("window must hold n_fft values")
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ssr_plan_create_ex(self.n_fft, self.hop, None if w is None else w.ctypes.data, int(self.center),
                                                   self._PAD[pad_mode], C.byref(h)))
            self.handle = h
            self._upload_tl_weights(w)
        self.fft_len, self.bluestein = 0, False
        self.lowpass_engine = "conv"

    def frames(self, n):
        pad = self.n_fft // 2 if self.center else 0
        return 0 if int(n) + 2 * pad < self.n_fft else 1 + (int(n) + 2 * pad - self.n_fft) // self.hop

    def check_lengths(self, lens_host):
        if not len(lens_host):
            return
        lo = int(np.min(lens_host))
        if self.center and self.pad_mode == "reflect" and lo <= self.n_fft // 2:
            raise ValueError("reflect padding needs every signal longer than n_fft//2 = %d samples" % (self.n_fft // 2))
        if lo < 1 or (not self.center and lo < self.n_fft):
            raise ValueError("every signal needs one whole frame (n_fft = %d samples without centring)" % self.n_fft)

    def set_lowpass_engine(self, engine):
        if engine != "conv":
            raise ValueError("a PlanEx has the conv engine only")
        return self


_ENGINES = {"segments": _lib.LOWPASS_SEGMENTS, "fused": _lib.LOWPASS_FUSED, "conv": _lib.LOWPASS_CONV}
_plans = {}
_plans_lock = threading.Lock()


_plans_ex = {}


def get_plan_ex(n_fft, hop, window_name, window, center, pad_mode, device=None):
    """The cached PlanEx of (n_fft, hop, window name, center, pad_mode, device); `window` = the float64 array of that name."""
    dev = torch.device(device) if device is not None else default_device()
    key = (int(n_fft), int(hop), window_name, bool(center), pad_mode, _device_index(dev))
    with _plans_lock:
        p = _plans_ex.get(key)
        if p is None:
            p = _plans_ex[key] = PlanEx(n_fft, hop, window, center, pad_mode, dev)
            p._cached = True
        return p


def get_plan(n_fft, hop, precision="f64", device=None, lowpass_engine="segments"):
    """The cached plan of (n_fft, hop, precision, device, low-pass engine)."""
    dev = torch.device(device) if device is not None else default_device()
    key = (int(n_fft), int(hop), _PREC[precision], _device_index(dev), lowpass_engine)
    with _plans_lock:
        p = _plans.get(key)
        if p is None:
            p = Plan(n_fft, hop, precision, dev)
            if lowpass_engine != "segments":
                p.set_lowpass_engine(lowpass_engine)
            p.lowpass_engine = lowpass_engine
            p._cached = True
            _plans[key] = p
        return p


class _DescRing:
    """Page-locked staging for the descriptor uploads (offsets, lengths, cut bins: a few KB per launch sequence): ONE 4 MB block used
    as a ring, so that an upload costs a memcpy and an asynchronous copy.  (tensor.pin_memory() per upload looked free and was not:
    while launches are queued ahead of the GPU every earlier staging block is still waiting for its copy, the caching host allocator
    has nothing to hand back and goes to hipHostMalloc - ~1 ms each, visible as idle gaps in front of every stage in the kernel
    trace.)  The ring has two halves; on entering a half the host waits for the events recorded when it last left it (one per stream
    that copied out of it) - hundreds of launch sequences earlier."""
    SIZE = 1 << 22
    _by_dev, _lock = {}, threading.Lock()

    def __init__(self):
        self.buf = torch.empty(self.SIZE, dtype=torch.uint8, pin_memory=True)
        self.host = self.buf.numpy()
        self.pos, self.half = 0, 0
        self.streams = {}                       # streams that copied out of the current half
        self.guard = [[], []]                   # events to wait for before a half is written again
        self.lock = threading.Lock()

    @classmethod
    def get(cls, idx):
        with cls._lock:
            r = cls._by_dev.get(idx)
            if r is None:
                r = cls._by_dev[idx] = cls()
            return r

    def stage(self, a, dev):
        """A page-locked copy of `a` that stays untouched until the current stream has passed what is queued next (a library
        call that reads host memory asynchronously: ssr_*_lsd_bands' edges)."""
        nbytes = a.nbytes
        room = (nbytes + 63) & ~63
        with self.lock:
            pos = self.pos
            if pos + room > (self.half + 1) * (self.SIZE // 2):          # leave this half: remember what must finish first
                evs = []
                for st in self.streams.values():
                    ev = torch.cuda.Event()
                    ev.record(st)
                    evs.append(ev)
                self.guard[self.half], self.streams = evs, {}
                self.half ^= 1
                pos = self.half * (self.SIZE // 2)
                for ev in self.guard[self.half]:
                    ev.synchronize()
                self.guard[self.half] = []
            self.pos = pos + room
            st = torch.cuda.current_stream(dev)
            self.streams[st.cuda_stream] = st
            self.host[pos:pos + nbytes] = a.reshape(-1).view(np.uint8)
            return self.buf[pos:pos + nbytes].view(_TORCH_OF[a.dtype.type]).view(a.shape)

    def put(self, a, dev):
        src = self.stage(a, dev)
        out = torch.empty(a.shape, dtype=src.dtype, device=dev)
        out.copy_(src, non_blocking=True)
        return out


_TORCH_OF = {np.int32: torch.int32, np.int64: torch.int64, np.float32: torch.float32, np.float64: torch.float64,
             np.int16: torch.int16, np.uint8: torch.uint8}


def _h2d(a, dev):
    """Host ndarray -> device tensor WITHOUT a stream synchronisation: through page-locked memory (_DescRing) and an asynchronous
    copy.  (A pageable source makes the runtime order the copy behind everything queued on the stream and makes the host wait for
    it - every descriptor upload was a full GPU drain: rocprofv3 showed an evaluate() pass with 42 ms of kernels in 65 ms of wall
    clock.)"""
    a = np.ascontiguousarray(a)
    dev = torch.device(dev)
    if dev.type != "cuda" or a.size == 0 or a.nbytes > _DescRing.SIZE // 8 or a.dtype.type not in _TORCH_OF:
        return torch.from_numpy(a).to(dev)
    with torch.cuda.device(dev):
        return _DescRing.get(torch.cuda.current_device()).put(a, dev)


def _host_i32(a, dev):
    """int32 array the library reads from HOST memory, as a host tensor: page-locked when it fits the ring (the library's copy
    out of it then stays asynchronous).  The caller keeps the tensor until the call that reads it has been queued."""
    a = np.ascontiguousarray(a, dtype=np.int32)
    if dev.type == "cuda" and 0 < a.nbytes <= _DescRing.SIZE // 8:
        with torch.cuda.device(dev):
            return _DescRing.get(torch.cuda.current_device()).stage(a, dev)
    return torch.from_numpy(a)


def _args(values):
    """Tensors -> their data pointers; everything else as it is."""
    return [_vp(v) if isinstance(v, torch.Tensor) else v for v in values]


def _is_f64(a):
    return (a.dtype == torch.float64) if isinstance(a, torch.Tensor) else (getattr(a, "dtype", None) == np.float64)


def _is_number(x):
    """A Python or NumPy real number; a bool is none."""
    return not isinstance(x, bool) and isinstance(x, (int, float, np.integer, np.floating))


def _number_in(x, lo, hi, lo_open, hi_open, message):
    """x as it is, or ValueError(message): a number (_is_number; NaN is outside) between lo and hi, either end open or closed."""
    if not _is_number(x) or not (lo < float(x) if lo_open else lo <= float(x)) or not (float(x) < hi if hi_open else float(x) <= hi):
        raise ValueError(message)
    return x


class Ragged:
    """A ragged batch of 1-D signals resident on the device: float32, or float64 where the reference would hold
    float64 (IIR-degraded / resampled-from-float64 estimates)."""

    def __init__(self, data, off, lens_dev, lens_host):
        self.data, self.off, self.len = data, off, lens_dev
        self.lens_host = np.asarray(lens_host, dtype=np.int64)
        self.n = len(self.lens_host)
        self.max_len = int(self.lens_host.max()) if self.n else 0
        self.device = data.device
        self.packed = True                      # the signals sit back to back in `data` (from_list(allow_gaps=True) may say otherwise)

    @staticmethod
    def from_list(arrays, device=None, dtype=torch.float32, allow_gaps=False):
        """allow_gaps (callers that only hand data / off / len to a kernel: the metric stage): views into ONE device buffer in
        increasing address order are taken where they lie even with unused samples between them - `off` says where each starts
        (est[:m] / target[:m] of metrics.py:89-90 cut a sample off an item here and there, which used to send the whole batch
        through a per-signal `.to()` and a concatenation).  Such a batch is not `packed`: split() refuses it."""
        dev = torch.device(device) if device is not None else default_device()
        arrays = list(arrays)
        if allow_gaps and len(arrays) > 1:
            g = Ragged._from_views_with_gaps(arrays, dev, dtype)
            if g is not None:
                return g
        # Views that already sit back to back in ONE device buffer (the output of an earlier launch: upload_decoded,
        # resample_sinc, fft_lowpass, resample_poly ...) are taken as they are: no per-signal transfer call, no concatenation.
        if len(arrays) > 1 and all(isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == dtype and a.dim() == 1 and a.is_contiguous()
                                   for a in arrays):
            # (address adjacency is NOT enough - two separate allocations are routinely back to back in the caching
            # allocator, and set_() past the end of a0's storage silently reallocates it: every view must live in a0's storage
            # and the whole run must fit inside it.)
            a0 = arrays[0]
            es, ok, end, st0 = a0.element_size(), True, a0.data_ptr(), a0.untyped_storage().data_ptr()
            for a in arrays:
                ok = ok and a.data_ptr() == end and a.device == a0.device and a.untyped_storage().data_ptr() == st0
                end += a.numel() * es
            ok = ok and end <= st0 + a0.untyped_storage().nbytes()
            if ok and arrays[0].device.index == (_device_index(dev)):
                lens = np.array([a.shape[0] for a in arrays], dtype=np.int64)
                total = int(lens.sum())
                if 0 < total and lens.max() < 2 ** 31:
                    a0 = arrays[0]
                    data = torch.empty(0, dtype=dtype, device=a0.device).set_(a0.untyped_storage(), a0.storage_offset(), (total,), (1,))
                    desc = _h2d(_offsets(lens), a0.device)
                    return Ragged(data, desc, _h2d(lens.astype(np.int32), a0.device), lens)
        ts = []
        for a in arrays:
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
            if t.dim() != 1:
                raise ValueError("expected 1-D signals, got shape %s" % (tuple(t.shape),))
            ts.append(t.to(device=dev, dtype=dtype, non_blocking=True))
        lens = np.array([t.shape[0] for t in ts], dtype=np.int64)
        if len(ts) and lens.max() >= 2 ** 31:
            raise ValueError("signal too long")
        data = torch.cat(ts) if len(ts) else torch.empty(0, dtype=dtype, device=dev)
        return Ragged(data, _h2d(_offsets(lens), dev), _h2d(lens.astype(np.int32), dev), lens)

    @staticmethod
    def _from_views_with_gaps(arrays, dev, dtype):
        a0 = arrays[0]
        if not (isinstance(a0, torch.Tensor) and a0.is_cuda):
            return None
        idx = _device_index(dev)
        es, st = a0.element_size(), a0.untyped_storage()
        st0, p0, end = st.data_ptr(), a0.data_ptr(), a0.data_ptr()
        off, lens = [], []
        for a in arrays:
            if not (isinstance(a, torch.Tensor) and a.dtype == dtype and a.dim() == 1 and a.is_contiguous() and a.device == a0.device
                    and a.untyped_storage().data_ptr() == st0):
                return None
            p = a.data_ptr()
            if p < end:                                  # out of order or overlapping: not this path
                return None
            off.append((p - p0) // es); lens.append(a.shape[0])
            end = p + a.shape[0] * es
        lens = np.array(lens, dtype=np.int64)
        if a0.device.index != idx or end > st0 + st.nbytes() or lens.sum() == 0 or lens.max() >= 2 ** 31:
            return None
        data = torch.empty(0, dtype=dtype, device=a0.device).set_(st, a0.storage_offset(), ((end - p0) // es,), (1,))
        r = Ragged(data, _h2d(np.array(off, dtype=np.int64), a0.device), _h2d(lens.astype(np.int32), a0.device), lens)
        r.packed = bool(off[-1] + lens[-1] == lens.sum())
        return r

    @staticmethod
    def from_list_keep64(arrays, device=None, allow_gaps=False):
        """float64 batch if ANY signal is float64 (exact for the float32 ones), else float32."""
        arrays = list(arrays)
        return Ragged.from_list(arrays, device, torch.float64 if any(_is_f64(a) for a in arrays) else torch.float32, allow_gaps)

    @staticmethod
    def from_uniform(x):
        """x: [N, n] float32 contiguous device tensor - no copy, descriptors built on the device."""
        if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
            raise ValueError("from_uniform needs a contiguous float32 [N, n] device tensor")
        N, n = x.shape
        return Ragged(x.view(-1), *_uniform_images(N, n, x.device), np.full(N, n, dtype=np.int64))

    def split(self, flat=None):
        if not self.packed:
            raise ValueError("a batch of views with gaps has no packed layout to split")
        flat = self.data if flat is None else flat
        o = np.concatenate(([0], np.cumsum(self.lens_host)))
        return [flat[o[i]:o[i + 1]] for i in range(self.n)]


class _Rows:
    """Row (frame) descriptors of a ragged batch under a plan."""

    def __init__(self, plan, lens_host, device):
        self.T = np.array([plan.frames(n) for n in lens_host], dtype=np.int64)
        self.total = int(self.T.sum())
        self.max_T = int(self.T.max()) if len(self.T) else 0
        self.off_host = _offsets(self.T)
        self.off = _h2d(self.off_host, device)


def _check_reflect(plan, lens_host):
    plan.check_lengths(lens_host)


def _check_nonempty(lens_host):
    """librosa-style reflect padding (numpy.pad) repeats the reflection for short signals; only empty ones fail."""
    if len(lens_host) and int(np.min(lens_host)) < 1:
        raise ValueError("empty signal")


# ------------------------------------------------------------------------------------------------------
class PairBatch:
    """(est, target) ragged batch + cached descriptors/workspace for repeated ssr_pair_metrics calls."""

    def __init__(self, plan, est, tgt):
        if est.n != tgt.n or not np.array_equal(est.lens_host, tgt.lens_host):
            raise ValueError("est and target must have identical lengths (truncate to min_len first)")
        _check_nonempty(est.lens_host)
        if tgt.data.dtype == torch.float64 and est.data.dtype != torch.float64:
            # float32 estimate against a float64 target: widening the estimate is exact, and the reference promotes
            # every mixed operation to float64 anyway
            est = Ragged(est.data.to(torch.float64), est.off, est.len, est.lens_host)
            self.est = est
        self.plan, self.est, self.tgt = plan, est, tgt
        self.rows = _Rows(plan, est.lens_host, est.device)
        # the workspace is allocated on first use for the mask at hand: without SSIM no magnitude image is materialised
        # (8 bytes per bin of the batch otherwise), and it only grows when a later call asks for more
        self.ws_bytes, self.ws, self._ws_mask = 0, None, 0
        self.out = torch.empty((est.n, 4), dtype=torch.float64, device=est.device)

    def _workspace(self, mask):
        if self.ws is None or (mask & ~self._ws_mask):
            want = mask | self._ws_mask
            p, e = self.plan, self.est
            self.ws_bytes = int(p.lib.ssr_pair_metrics_workspace_bytes_for(p.handle, e.n, e.max_len, self.rows.total, want))
            self.ws = None                                          # release before the larger allocation
            self.ws = _workspace(self.ws_bytes, e.device)
            self._ws_mask = want

    def run(self, mask=M_ALL, stages=7):
        p, e, t = self.plan, self.est, self.tgt
        if e.n == 0:
            return self.out
        self._workspace(mask)
        if (mask & M_SSIM) and (self.rows.T.min() < 7 or p.n_bins < 7):
            raise ValueError("win_size exceeds image extent")  # what skimage raises for images smaller than 7x7
        if e.data.dtype == torch.float64:
            if stages != 7:
                raise ValueError("stage selection is a bench facility of the float32 path")
            fn = p.lib.ssr_pair_metrics_f64 if t.data.dtype == torch.float64 else p.lib.ssr_pair_metrics_est64
            _lib.check(fn(
                p.handle, _vp(e.data), _vp(e.off), _vp(t.data), _vp(t.off), _vp(e.len), _vp(self.rows.off), e.n,
                e.max_len, self.rows.total, mask, _vp(self.out), _vp(self.ws), self.ws_bytes, _stream()))
            return self.out
        _lib.check(p.lib.ssr_pair_metrics_stages(
            p.handle, _vp(e.data), _vp(e.off), _vp(t.data), _vp(t.off), _vp(e.len), _vp(self.rows.off), e.n, e.max_len,
            self.rows.total, mask, _vp(self.out), _vp(self.ws), self.ws_bytes, _stream(), stages))
        return self.out


class MultiPairBatch:
    """ONE target, K estimates per item (ssr_pair_metrics_multi): `est` holds n_keys * n items KEY-MAJOR (estimate k of item i
    at index k * n + i), every estimate of item i as long as target i.  The target is transformed once and its magnitude image
    stored once; estimates 1 .. K-1 are transformed two per complex transform.  out: [n, n_keys, 4] float64.
    A float64 `est` against a float32 target (every IIR key of a file, ssr_eval/eval.py:243-258): ssr_pair_metrics_multi_est64."""

    def __init__(self, plan, est, tgt, n_keys):
        n_keys = int(n_keys)
        if n_keys < 1 or est.n != tgt.n * n_keys or not np.array_equal(est.lens_host, np.tile(tgt.lens_host, n_keys)):
            raise ValueError("est must hold n_keys estimates per target, key-major, each as long as its target")
        if tgt.data.dtype != torch.float32 or est.data.dtype not in (torch.float32, torch.float64):
            raise ValueError("ssr_pair_metrics_multi takes float32 targets and float32 or float64 estimates (float64 targets go through PairBatch)")
        _check_nonempty(tgt.lens_host)
        self.plan, self.est, self.tgt, self.n_keys = plan, est, tgt, n_keys
        self.est64 = est.data.dtype == torch.float64
        self.rows = _Rows(plan, tgt.lens_host, tgt.device)
        self.ws_bytes, self.ws, self._ws_mask = 0, None, 0
        self.out = torch.empty((tgt.n, n_keys, 4), dtype=torch.float64, device=tgt.device)

    def _workspace(self, mask):
        if self.ws is None or (mask & ~self._ws_mask):
            want = mask | self._ws_mask
            p, t = self.plan, self.tgt
            size_fn = p.lib.ssr_pair_metrics_multi_est64_workspace_bytes if self.est64 else p.lib.ssr_pair_metrics_multi_workspace_bytes
            self.ws_bytes = int(size_fn(p.handle, t.n, self.n_keys, t.max_len, self.rows.total, want))
            self.ws = None
            self.ws = _workspace(self.ws_bytes, t.device)
            self._ws_mask = want

    def run(self, mask=M_ALL):
        p, e, t = self.plan, self.est, self.tgt
        if t.n == 0:
            return self.out
        self._workspace(mask)
        if (mask & M_SSIM) and (self.rows.T.min() < 7 or p.n_bins < 7):
            raise ValueError("win_size exceeds image extent")
        fn = p.lib.ssr_pair_metrics_multi_est64 if self.est64 else p.lib.ssr_pair_metrics_multi
        _lib.check(fn(
            p.handle, _vp(e.data), _vp(e.off), _vp(t.data), _vp(t.off), _vp(t.len), _vp(self.rows.off), t.n, self.n_keys, t.max_len,
            self.rows.total, mask, _vp(self.out), _vp(self.ws), self.ws_bytes, _stream()))
        return self.out


class Pending:
    """A device result on its way to the host: the copy into page-locked memory is queued behind the launch sequence that produces
    it, and calling the object waits for THAT copy only (an event) and returns the ndarray - the host can queue the next batch's
    launches in between.  The page-locked buffers come from a small free list: with launches queued ahead torch's caching
    host allocator has no block whose event has completed and falls back to hipHostMalloc (~1 ms per result, the gap _DescRing removed
    from the uploads); a buffer returns to the list when its result has been taken."""

    _free = {}                 # bytes (rounded up to 4 KiB) -> [page-locked uint8 tensors]
    _KEEP = 8                  # per size class

    @classmethod
    def _take(cls, nbytes):
        size = max(4096, (nbytes + 4095) & ~4095)
        lst = cls._free.setdefault(size, [])
        return size, (lst.pop() if lst else torch.empty(size, dtype=torch.uint8, pin_memory=True))

    def __init__(self, t):
        t = t.contiguous()
        nbytes = t.numel() * t.element_size()
        self._size, self._buf = self._take(nbytes)
        self.host = self._buf[:nbytes].view(t.dtype).view(t.shape)
        self.host.copy_(t, non_blocking=True)
        self.ev = torch.cuda.Event()
        self.ev.record(torch.cuda.current_stream(t.device))
        self._value = None

    def __call__(self):
        if self._value is None:
            self.ev.synchronize()
            self._value = self.host.numpy().copy()          # the caller's array does not alias the recycled buffer
            lst = self._free.setdefault(self._size, [])
            if len(lst) < self._KEEP:
                lst.append(self._buf)
            self._buf = self.host = None
        return self._value


def pair_metrics_multi(plan, est_lists, tgt_list, mask=M_ALL, deferred=False):
    """est_lists: K lists (one per key) of n waveforms - all float32, or all float64 (the IIR keys of a file: they stay float64, as in the
    reference); tgt_list: n float32 targets -> [n, K, 4] float64 (deferred: a Pending)."""
    with torch.cuda.device(plan.device):
        flat = [e for key in est_lists for e in key]
        b = MultiPairBatch(plan, Ragged.from_list_keep64(flat, plan.device, allow_gaps=True), Ragged.from_list(tgt_list, plan.device, allow_gaps=True),
                           len(est_lists))
        return Pending(b.run(mask)) if deferred else b.run(mask).cpu().numpy()


def pair_metrics(plan, est_list, tgt_list, mask=M_ALL, deferred=False):
    """[n, 4] float64 (lsd, log_sispec, sispec, ssim) for lists of equal-length (est, target) waveforms.
    float64 signals stay float64 (ssr_pair_metrics_est64 / ssr_pair_metrics_f64).  deferred: a Pending instead of the ndarray."""
    with torch.cuda.device(plan.device):
        b = PairBatch(plan, Ragged.from_list_keep64(est_list, plan.device, allow_gaps=True),
                      Ragged.from_list_keep64(tgt_list, plan.device, allow_gaps=True))
        return Pending(b.run(mask)) if deferred else b.run(mask).cpu().numpy()


# ---- band-split LSD ---------------------------------------------------------------------------------------------------------
# Bytes of magnitude images one ssr_pair_lsd_bands call may hold (_pair_keys_chunked: the keys run in chunks whose images fit).
LSD_BANDS_WS_BYTES = 1 << 30


def _pair_keys_chunked(plan, est_lists, tgt_list, n_cols, budget, keys_per_chunk, f64_target_error, ws_bytes_of, entries, extra,
                       deferred):
    """The multi-key pair calls that hold K + 1 magnitude images per item (8 bytes per bin of the batch per key - more than HBM holds
    for 36 keys of a large batch): the keys run in chunks of keys_per_chunk, or as many as fit in `budget` bytes of images (a
    multiple of six where more than six fit: whole groups of the reduction's three keys per wave), every chunk against the same
    targets.  ws_bytes_of(n, keys, max_len, total_rows) sizes the workspace, entries = (float32-estimate, float64-estimate) entry
    points, extra(k0, k1) -> the arguments between total_rows and out for keys k0 .. k1 - 1.
    -> [n, K, n_cols] float64 (deferred: a Pending)."""
    K, n = len(est_lists), len(tgt_list)
    with torch.cuda.device(plan.device):
        tgt = Ragged.from_list(tgt_list, plan.device, allow_gaps=True)
        if any(_is_f64(t) for t in tgt_list):
            raise ValueError(f64_target_error)
        _check_nonempty(tgt.lens_host)
        rows = _Rows(plan, tgt.lens_host, tgt.device)
        out = torch.empty((n, K, n_cols), dtype=torch.float64, device=tgt.device)
        if n and K:
            if keys_per_chunk is None:
                plane = rows.total * ((plan.n_bins + 3) & ~3) * 4
                keys_per_chunk = max(1, budget // max(plane, 1) - 1)
                if keys_per_chunk > 6:
                    keys_per_chunk -= keys_per_chunk % 6
            kc = max(1, min(int(keys_per_chunk), K))
            ws_bytes = int(ws_bytes_of(n, kc, tgt.max_len, rows.total))
            ws = _workspace(ws_bytes, tgt.device)
            for k0 in range(0, K, kc):
                k1 = min(K, k0 + kc)
                est = Ragged.from_list_keep64([w for key in est_lists[k0:k1] for w in key], plan.device, allow_gaps=True)
                if not np.array_equal(est.lens_host, np.tile(tgt.lens_host, k1 - k0)):
                    raise ValueError("every estimate must be as long as its target (truncate to min_len first)")
                o = out if k1 - k0 == K else torch.empty((n, k1 - k0, n_cols), dtype=torch.float64, device=tgt.device)
                args = extra(k0, k1)
                _lib.check(entries[est.data.dtype == torch.float64](
                    plan.handle, _vp(est.data), _vp(est.off), _vp(tgt.data), _vp(tgt.off), _vp(tgt.len), _vp(rows.off), n, k1 - k0,
                    tgt.max_len, rows.total, *_args(args), _vp(o), _vp(ws), ws_bytes, _stream()))
                if o is not out:
                    out[:, k0:k1] = o
        return Pending(out) if deferred else out.cpu().numpy()


def _image_pairs(name, est, target, n_bins, extra):
    """The image-level entry points ssr_spectrogram_<name> on est / target: [N, T, F] magnitude images (float32, on one device).
    n_bins: the F a mel family's filterbank asks for - those families skip an empty batch and refuse images without rows here - or
    None.  extra(N, F, dev) -> (columns of `out`, the query's arguments after max_rows, the call's arguments between n_bins and
    out: a tensor among them passes its pointer and lives until the call is queued).  -> [N, columns] float64 device tensor."""
    require_gpu()
    lib = _lib.load()
    dev = est.device if isinstance(est, torch.Tensor) and est.is_cuda else default_device()
    with torch.cuda.device(dev):
        x = _dev_f32(est, dev).contiguous()
        y = _dev_f32(target, dev).contiguous()
        if x.dim() != 3 or x.shape != y.shape or (n_bins is not None and int(x.shape[2]) != n_bins):
            raise ValueError("spectrogram shape mismatch: %s vs %s" % (tuple(x.shape), tuple(y.shape)) if n_bins is None else
                             "expected two [N, T, %d] images, got %s and %s" % (n_bins, tuple(x.shape), tuple(y.shape)))
        N, T, F = (int(v) for v in x.shape)
        cols, ws_args, args = extra(N, F, dev)
        out = torch.empty((N, cols), dtype=torch.float64, device=dev)
        if N or n_bins is None:
            if T < 1 and n_bins is not None:
                raise ValueError("empty spectrogram")
            off, rows = _uniform_images(N, T, dev)
            ws_bytes = int(getattr(lib, "ssr_spectrogram_%s_workspace_bytes" % name)(N, T, *ws_args))
            ws = _workspace(ws_bytes, dev)
            _lib.check(getattr(lib, "ssr_spectrogram_" + name)(_vp(x), _vp(off), _vp(y), _vp(off), _vp(rows), N, T, F, *_args(args), _vp(out),
                                                               _vp(ws), ws_bytes, _stream()))
        return out


def spectrogram_lsd_bands(est, target, edges):
    """est / target: [N, T, F] magnitude images (float32, on one device), edges: int [N][n_bands + 1] -> [N, n_bands] float64 device
    tensor (ssr_spectrogram_lsd_bands)."""
    def extra(N, F, dev):
        e = np.asarray(edges, dtype=np.int32)
        if e.ndim != 2 or e.shape[0] != N:
            raise ValueError("edges must be [n_images][n_bands + 1]")
        nb = e.shape[1] - 1
        if nb < 1:
            raise ValueError("at least one band (two edges) per image")
        return nb, (nb,), (_host_i32(e, dev), nb)
    return _image_pairs("lsd_bands", est, target, None, extra)


def pair_lsd_bands(plan, est_lists, tgt_list, edges, deferred=False, keys_per_chunk=None):
    """Band LSDs of K estimates per target: est_lists = K lists of n waveforms (all float32 or all float64, each as long as its
    target), tgt_list = n float32 targets, edges: int [K][n][n_bands + 1] -> [n, K, n_bands] float64 (deferred: a Pending).
    The keys run in chunks (_pair_keys_chunked: keys_per_chunk, or as many as fit in LSD_BANDS_WS_BYTES)."""
    K, n = len(est_lists), len(tgt_list)
    e = np.asarray(edges, dtype=np.int32)
    if e.ndim != 3 or e.shape[:2] != (K, n):
        raise ValueError("edges must be [n_keys][n_items][n_bands + 1]")
    nb = e.shape[2] - 1
    if nb < 1:
        raise ValueError("at least one band (two edges) per image")
    lib = plan.lib
    return _pair_keys_chunked(plan, est_lists, tgt_list, nb, LSD_BANDS_WS_BYTES, keys_per_chunk,
                              "band LSD takes float32 targets (float64 estimates are kept float64)",
                              lambda n, kc, max_len, total: lib.ssr_pair_lsd_bands_workspace_bytes(plan.handle, n, kc, max_len, total, nb),
                              (lib.ssr_pair_lsd_bands, lib.ssr_pair_lsd_bands_est64),
                              lambda k0, k1: (_host_i32(e[k0:k1], plan.device), nb), deferred)


# ---- STOI / ESTOI ----------------------------------------------------------------------------------------------------------
STOI_FS = 10000                  # pystoi's analysis rate


# ---- mel-spectrogram distances ----------------------------------------------------------------------------------------------
# Bytes of magnitude images one ssr_pair_mel_metrics call may hold (as LSD_BANDS_WS_BYTES: the keys run in chunks that fit).
MEL_WS_BYTES = 1 << 30


def _fb_arg(fb):
    """fb: a float32 [n_bins, n_mels] torch-CPU tensor the caller keeps unchanged (AudioMetrics caches it page-locked: the library's
    copy out of it is then asynchronous) -> (n_bins, n_mels, pointer)."""
    if not isinstance(fb, torch.Tensor) or fb.dtype != torch.float32 or fb.dim() != 2 or fb.is_cuda or not fb.is_contiguous():
        raise ValueError("the filterbank must be a contiguous float32 [n_bins, n_mels] host tensor")
    return int(fb.shape[0]), int(fb.shape[1]), C.c_void_p(fb.data_ptr())


def spectrogram_mel(sp, fb):
    """sp: [N, T, F] magnitude images (float32, one device), fb: [F, n_mels] host float32 -> [N, T, n_mels] float32 device tensor
    (ssr_spectrogram_mel)."""
    require_gpu()
    lib = _lib.load()
    dev = sp.device if isinstance(sp, torch.Tensor) and sp.is_cuda else default_device()
    nb, nm, fp = _fb_arg(fb)
    with torch.cuda.device(dev):
        x = _dev_f32(sp, dev).contiguous()
        if x.dim() != 3 or int(x.shape[2]) != nb:
            raise ValueError("expected [N, T, %d] images, got %s" % (nb, tuple(x.shape)))
        N, T, F = (int(v) for v in x.shape)
        out = torch.empty((N, T, nm), dtype=torch.float32, device=dev)
        if N and T:
            off, rows = _uniform_images(N, T, dev)
            ws_bytes = int(lib.ssr_spectrogram_mel_workspace_bytes(F, nm))
            ws = _workspace(ws_bytes, dev)
            _lib.check(lib.ssr_spectrogram_mel(_vp(x), _vp(off), _vp(rows), N, T, F, fp, nm, _vp(out), _vp(ws), ws_bytes, _stream()))
        return out


def spectrogram_mel_metrics(est, target, fb, n_cep, which):
    """est / target: [N, T, F] magnitude images -> [N, 3] float64 device tensor (mel_lsd, mel_l1, mcd; NaN where `which` does not
    ask; ssr_spectrogram_mel_metrics)."""
    nb, nm, fp = _fb_arg(fb)
    return _image_pairs("mel_metrics", est, target, nb, lambda N, F, dev: (3, (F, nm, int(n_cep)), (fp, nm, int(n_cep), int(which))))


def pair_mel_metrics(plan, est_lists, tgt_list, fb, n_cep, which, deferred=False, keys_per_chunk=None):
    """Mel distances of K estimates per target: est_lists = K lists of n waveforms (all float32 or all float64, each as long as its
    target), tgt_list = n float32 targets, fb: [plan.n_bins, n_mels] host float32 -> [n, K, 3] float64 (deferred: a Pending).
    The keys run in chunks as in pair_lsd_bands (keys_per_chunk, or as many as fit in MEL_WS_BYTES)."""
    nb, nm, fp = _fb_arg(fb)
    if nb != plan.n_bins:
        raise ValueError("the filterbank has %d bins, the transform %d" % (nb, plan.n_bins))
    lib = plan.lib
    return _pair_keys_chunked(plan, est_lists, tgt_list, 3, MEL_WS_BYTES, keys_per_chunk,
                              "mel distances take float32 targets (float64 estimates are kept float64)",
                              lambda n, kc, max_len, total: lib.ssr_pair_mel_metrics_workspace_bytes(plan.handle, n, kc, max_len, total, nm,
                                                                                                     int(n_cep)),
                              (lib.ssr_pair_mel_metrics, lib.ssr_pair_mel_metrics_est64),
                              lambda k0, k1: (fp, nm, int(n_cep), int(which)), deferred)


def spectrogram_mel_dtw(est, target, fb, n_cep, radius):
    """est / target: [N, T, F] magnitude images -> [N, 3] float64 device tensor (mcd_dtw, dtw_dev, dtw_len; ssr_spectrogram_mel_dtw)."""
    nb, nm, fp = _fb_arg(fb)
    return _image_pairs("mel_dtw", est, target, nb, lambda N, F, dev: (3, (F, nm, int(n_cep), int(radius)), (fp, nm, int(n_cep), int(radius))))


def pair_mel_dtw(plan, est_lists, tgt_list, fb, n_cep, radius, deferred=False, keys_per_chunk=None):
    """DTW-aligned mel-cepstral distortion of K estimates per target, with pair_mel_metrics' arguments and key chunking (radius in
    frames for `which`) -> [n, K, 3] float64: mcd_dtw, dtw_dev, dtw_len (deferred: a Pending)."""
    nb, nm, fp = _fb_arg(fb)
    if nb != plan.n_bins:
        raise ValueError("the filterbank has %d bins, the transform %d" % (nb, plan.n_bins))
    lib = plan.lib
    return _pair_keys_chunked(plan, est_lists, tgt_list, 3, MEL_WS_BYTES, keys_per_chunk,
                              "mel distances take float32 targets (float64 estimates are kept float64)",
                              lambda n, kc, max_len, total: lib.ssr_pair_mel_dtw_workspace_bytes(plan.handle, n, kc, max_len, total, nm,
                                                                                                 int(n_cep), int(radius)),
                              (lib.ssr_pair_mel_dtw, lib.ssr_pair_mel_dtw_est64),
                              lambda k0, k1: (fp, nm, int(n_cep), int(radius)), deferred)


def octave_taps(p, q):
    """The filter of pystoi.utils.resample_oct for resample_poly(x, p, q) (p / q reduced): Octave's resample() design - a
    Kaiser-windowed ideal low-pass at 1 / (2 max(p, q)) with 60 dB rejection - normalised to unit sum.  float64."""
    stop = 1.0 / (2 * max(p, q))
    roll = stop / 10
    rej_db = 60.0
    L = int(np.ceil((rej_db - 8) / (28.714 * roll)))
    t = np.arange(-L, L + 1)
    ideal = 2 * p * stop * np.sinc(2 * stop * t)
    h = np.kaiser(2 * L + 1, 0.1102 * (rej_db - 8.7)) * ideal
    return h / np.sum(h)


class StoiResamplePlan:
    """scipy.signal.resample_poly(x, 10000, fs, window=octave_taps(...)) as ssr_resample_poly_f64 runs it: with an array window
    SciPy keeps the taps float64 (a float32 signal is resampled in float64), half_len = (len(h) - 1) // 2 and h *= up.
    Cached per (rate, device), like ResamplePlan.get."""

    _cache = {}

    def __init__(self, fs, device):
        g = math.gcd(STOI_FS, int(fs))
        self.up, self.down = STOI_FS // g, int(fs) // g
        self.identity = self.up == 1 and self.down == 1      # scipy returns x.copy(); pystoi does not resample at all
        if self.identity:
            self.half_len = self.n_pre_pad = self.n_pre_remove = 0
            self.taps_host, self.taps64 = None, None
            return
        h = octave_taps(self.up, self.down) * self.up
        self.half_len = (len(h) - 1) // 2
        self.n_pre_pad = self.down - self.half_len % self.down
        self.n_pre_remove = (self.half_len + self.n_pre_pad) // self.down
        self.taps_host = np.concatenate((np.zeros(self.n_pre_pad), h))
        self.taps64 = torch.from_numpy(self.taps_host).to(device)

    @classmethod
    def get(cls, fs, device):
        key = (int(fs), str(device))
        p = cls._cache.get(key)
        if p is None:
            p = cls._cache[key] = cls(fs, device)
        return p

    def n_out(self, n_in):
        return int(n_in) if self.identity else -(-int(n_in) * self.up // self.down)

    def n_post_pad(self, n_in):
        """SciPy's trailing zero taps (they add nothing to the kept outputs; the device kernel reads zeros past the table)."""
        out_len = lambda nh: ((int(n_in) - 1) * self.up + nh - 1) // self.down + 1     # noqa: E731  (upfirdn's _output_len)
        n = 0
        while out_len(len(self.taps_host) + n) < self.n_out(n_in) + self.n_pre_remove:
            n += 1
        return n


def _resample_f64(wavs, plan, dev):
    """[float32 / float64 waveforms] (or a float64 Ragged) -> Ragged float64, resampled in float64 under `plan` (a StoiResamplePlan
    or a ResamplePlan: up, down, taps64, n_pre_remove, n_out) in one ssr_resample_poly_f64 launch; the identity plan returns the
    input batch itself, widened."""
    r = wavs if isinstance(wavs, Ragged) else Ragged.from_list(list(wavs), dev, torch.float64)
    if plan.identity:
        return r
    out_len = np.array([plan.n_out(n) for n in r.lens_host], dtype=np.int64)
    out = torch.empty(int(out_len.sum()), dtype=torch.float64, device=dev)
    out_off_d, out_len_d = _h2d(_offsets(out_len), dev), _h2d(out_len.astype(np.int32), dev)
    if r.n and out_len.max() > 0:
        _lib.check(_lib.load().ssr_resample_poly_f64(_vp(r.data), _vp(r.off), _vp(r.len), _vp(out_off_d), _vp(out_len_d), r.n,
                                                     int(out_len.max()), plan.up, plan.down, _vp(plan.taps64), int(plan.taps64.numel()),
                                                     plan.n_pre_remove, _vp(out), _stream()))
    return Ragged(out, out_off_d, out_len_d, out_len)


def resample_to_stoi_rate(wavs, fs, device=None):
    """The 10 kHz float64 signals pystoi analyses: [float32 / float64 waveforms at fs] -> Ragged float64 (ssr_resample_poly_f64 with
    the Octave taps; bit-identical to scipy.signal.resample_poly(x, 10000, fs, window=h))."""
    dev = torch.device(device) if device is not None else default_device()
    with torch.cuda.device(dev):
        return _resample_f64(wavs, StoiResamplePlan.get(fs, dev), dev)


# ---- the per-pair metric families: estimate e against target tgt_index[e] ------------------------------------------------------
def _ragged_where_they_lie(arrays, dev, dtype):
    """(data, off, lens_host) of a list of signals for a kernel that only reads them: device views of one buffer are taken where
    they lie in ANY order (from_list(allow_gaps=True) reads them in address order; the offsets are put back in list order), other
    inputs are packed as from_list packs them.  off: device int64 [n], item i at data + off[i]."""
    n = len(arrays)
    order = list(range(n))
    if n > 1 and all(isinstance(a, torch.Tensor) and a.is_cuda for a in arrays):
        order.sort(key=lambda i: arrays[i].data_ptr())
    r = Ragged.from_list([arrays[i] for i in order], dev, dtype, allow_gaps=True)
    if order == list(range(n)):
        return r.data, r.off, r.lens_host
    inv = np.argsort(np.asarray(order, np.int64))
    return r.data, r.off[_h2d(inv, r.device)], r.lens_host[inv]


def _placed_where_they_lie(tgts, ests, idx, dev):
    """The signals as ssr_wave_metrics / ssr_quality_metrics take them - (data, is-float64 flag, offsets) per side, read in their own
    dtype (a list holding both dtypes is widened to float64) -> (target side, estimate side, target lengths, estimate lengths)."""
    (tgt_side, tl), (est_side, el) = _placed_signals(tgts, dev), _placed_signals(ests, dev)
    return tgt_side, est_side, tl, el


def _placed_signals(wavs, dev):
    """One list of signals as _placed_where_they_lie places a side -> ((data, is-float64 flag, offsets), lengths)."""
    f64 = any(_is_f64(w) for w in wavs)
    data, off, lens = _ragged_where_they_lie(wavs, dev, torch.float64 if f64 else torch.float32)
    return (data, int(f64), off), lens


def _placed_resampled(r, n_t):
    """The signals as ssr_stoi / ssr_f0_metrics take them - (data, offsets) per side of ONE float64 batch r that holds the n_t
    targets, then the estimates (resampled together, in one launch) -> as _placed_where_they_lie."""
    return (r.data, r.off), (r.data, r.off[n_t:]), r.lens_host[:n_t], r.lens_host[n_t:]


def _signal_pair_index(tgt_list, est_list, tgt_index):
    """What a call on n_tgt targets and n_est >= 0 estimates checks before it needs a device -> (targets, estimates, tgt_index as
    int32 [n_est]), or ValueError."""
    tgts, ests = list(tgt_list), list(est_list)
    idx = np.asarray(tgt_index, dtype=np.int32).reshape(-1)
    if idx.shape[0] != len(ests):
        raise ValueError("one target index per estimate")
    if len(ests) and (idx.min() < 0 or idx.max() >= len(tgts)):
        raise ValueError("tgt_index out of range")
    return tgts, ests, idx


def _split_array(split, n_e, valid, message):
    """A call's split per estimate as int32 [n_est] (None: -1, no split, for every estimate), or ValueError(message) unless it holds
    one entry per estimate and valid(array): the bound is the family's own."""
    sp = np.full(n_e, -1, np.int32) if split is None else np.asarray(split, dtype=np.int32).reshape(-1)
    if sp.shape[0] != n_e or (n_e and not valid(sp)):
        raise ValueError(message)
    return sp


def _gpu_call(device):
    """-> (the library, the device of the call), or RuntimeError without a GPU: what every argument check of a call comes before."""
    require_gpu()
    return _lib.load(), torch.device(device) if device is not None else default_device()


def _signal_pair_place(tgts, ests, idx, dev):
    """The n_tgt >= 1 targets and n_est >= 0 estimates of _signal_pair_index on the device -> (target side, estimate side, target
    lengths): as _placed_where_they_lie places them, every estimate as long as its target; without estimates the targets alone."""
    if not ests:
        tgt_side, tl = _placed_signals(tgts, dev)
        return tgt_side, (None, 0, None), tl
    tgt_side, est_side, tl, el = _placed_where_they_lie(tgts, ests, idx, dev)
    if not np.array_equal(el, tl[idx]):
        raise ValueError("every estimate must be as long as its target (truncate to the common length first)")
    return tgt_side, est_side, tl


def _hop_blocks(tl, hop, limit):
    """Whole blocks of `hop` samples per signal (none below two), or ValueError where a signal holds more than `limit`."""
    blocks = np.where(tl >= 2 * hop, tl // hop, 0)
    if blocks.max() > limit:
        raise ValueError("a signal may hold at most %d blocks of %d samples" % (limit, hop))
    return blocks


def _take(t):
    """A device result on its way to the host, as a function that returns the array: a Pending, or for an empty tensor - nothing
    was computed - an empty array of its shape."""
    return Pending(t) if t.numel() else (lambda: np.empty(tuple(t.shape)))


def _collected(got, deferred):
    """The tuple of what the functions `got` return (deferred: the function that returns it)."""
    collect = lambda: tuple(g() for g in got)      # noqa: E731
    return collect if deferred else collect()


def _pair_index_metrics(tgt_list, est_list, tgt_index, n_cols, place, ws_bytes_of, entry, scalars, device, deferred):
    """One call of a per-pair family: estimate e is scored against target tgt_index[e], every estimate as long as its target ->
    [n_est, n_cols] float64 (deferred: a Pending).  place(targets, estimates, tgt_index, dev) puts the signals on the device (see
    _placed_*).  The C ABI's calls share one shape: ws_bytes_of(tgt_len, n_tgt, tgt_index, n_est) and entry(target side ...,
    tgt_len, n_tgt, estimate side ..., tgt_index, n_est, scalars ..., out, workspace, bytes, stream), with tgt_len and tgt_index
    int32 arrays in HOST memory."""
    require_gpu()
    dev = torch.device(device) if device is not None else default_device()
    n_t, n_e = len(tgt_list), len(est_list)
    idx = np.asarray(tgt_index, dtype=np.int32).reshape(-1)
    if idx.shape[0] != n_e:
        raise ValueError("one target index per estimate")
    with torch.cuda.device(dev):
        out = torch.empty((n_e, n_cols), dtype=torch.float64, device=dev)
        if n_e:
            if idx.min() < 0 or idx.max() >= n_t:
                raise ValueError("tgt_index out of range")
            tgt_side, est_side, tl, el = place(list(tgt_list), list(est_list), idx, dev)
            if not np.array_equal(el, tl[idx]):
                raise ValueError("every estimate must be as long as its target (truncate to the common length first)")
            lens = tl.astype(np.int32)
            ws_bytes = int(ws_bytes_of(lens.ctypes.data_as(C.c_void_p), n_t, idx.ctypes.data_as(C.c_void_p), n_e))
            ws = _workspace(ws_bytes, dev)
            lens_h, idx_h = _host_i32(lens, dev), _host_i32(idx, dev)
            _lib.check(entry(*_args(tgt_side), _vp(lens_h), n_t, *_args(est_side), _vp(idx_h), n_e, *scalars, _vp(out), _vp(ws), ws_bytes,
                             _stream()))
        return Pending(out) if deferred else out.cpu().numpy()


def stoi(tgt_list, est_list, tgt_index, fs, which=_lib.STOI, device=None, deferred=False):
    """STOI / ESTOI of estimate e against target tgt_index[e] (ssr_stoi): waveforms at `fs` (float32 or float64, each estimate as
    long as its target) -> [n_est, n_out] float64 (which = STOI_BOTH: columns STOI, ESTOI).  Targets and estimates are resampled to
    10 kHz in one launch; each target's mask and band image are computed once for all its estimates.  deferred: a Pending."""
    lib = _lib.load()

    def place(tgts, ests, idx, dev):
        # the lengths are compared (and the estimates' own passed to the library) AFTER resampling
        tgt_side, est_side, tl, el = _placed_resampled(resample_to_stoi_rate(tgts + ests, fs, dev), len(tgts))
        return tgt_side, est_side + (_host_i32(el, dev),), tl, el
    return _pair_index_metrics(tgt_list, est_list, tgt_index, 2 if which == _lib.STOI_BOTH else 1, place, lib.ssr_stoi_workspace_bytes,
                               lib.ssr_stoi, (int(which),), device, deferred)


# ---- waveform metrics: SNR, SI-SDR, segmental SNR ----------------------------------------------------------------------------
def wave_metrics(tgt_list, est_list, tgt_index, fs, which=7, device=None, deferred=False):
    """SNR / SI-SDR / segmental SNR of estimate e against target tgt_index[e] (ssr_wave_metrics): waveforms at `fs`
    (float32 or float64, each estimate as long as its target; a list holding both dtypes is widened to float64) -> [n_est, n_out]
    float64, columns in bit order of `which` (1 snr, 2 si_sdr, 4 seg_snr).  Device views of one buffer are read where they lie;
    pairs next to each other that name one target read its tiles once.  deferred: a Pending."""
    which = int(which)
    if not 1 <= which <= 7:
        raise ValueError("which must be a non-empty combination of 1 (snr), 2 (si_sdr) and 4 (seg_snr)")
    lib = _lib.load()
    return _pair_index_metrics(tgt_list, est_list, tgt_index, bin(which).count("1"), _placed_where_they_lie,
                               lambda *a: lib.ssr_wave_metrics_workspace_bytes(*a, int(fs), which), lib.ssr_wave_metrics,
                               (int(fs), which), device, deferred)


# ---- objective quality measures: LLR, LPC cepstral distance, WSS, fwSNRseg ------------------------------------------------------
def quality_bands(fs):
    """(n_fft, cent [25], bw [25], filters [25, n_fft // 2]) float64: the critical bands and filters ssr_quality_metrics uses at fs."""
    lib = _lib.load()
    n = C.c_int32(0)
    _lib.check(lib.ssr_quality_bands(int(fs), C.byref(n), None, None, None, 0))
    cent, bw = np.zeros(25), np.zeros(25)
    filt = np.zeros((25, n.value // 2))
    _lib.check(lib.ssr_quality_bands(int(fs), C.byref(n), cent.ctypes.data_as(C.c_void_p), bw.ctypes.data_as(C.c_void_p),
                                     filt.ctypes.data_as(C.c_void_p), filt.size))
    return n.value, cent, bw, filt


def quality_metrics(tgt_list, est_list, tgt_index, fs, which=15, lpc_order=0, device=None, deferred=False):
    """LLR / cepstral distance / WSS / fwSNRseg of estimate e against target tgt_index[e] (ssr_quality_metrics):
    waveforms at `fs` (float32 or float64, each estimate as long as its target; a list holding both dtypes is widened to float64)
    -> [n_est, n_out] float64, columns in bit order of `which` (1 llr, 2 cep_dist, 4 wss, 8 fwseg_snr).  lpc_order 0: 10 below
    10 kHz, else 16.  Device views of one buffer are read where they lie; pairs next to each other that name one target analyse
    its frames once.  deferred: a Pending."""
    which, lpc_order = int(which), int(lpc_order)
    if not 1 <= which <= 15:
        raise ValueError("which must be a non-empty combination of 1 (llr), 2 (cep_dist), 4 (wss) and 8 (fwseg_snr)")
    if not 0 <= lpc_order <= 32:
        raise ValueError("lpc_order must be 0 (default) or in [1, 32]")
    if not 8000 <= int(fs) <= 48000:
        raise ValueError("the quality measures need 8000 <= fs <= 48000")
    lib = _lib.load()
    return _pair_index_metrics(tgt_list, est_list, tgt_index, bin(which).count("1"), _placed_where_they_lie,
                               lambda *a: lib.ssr_quality_metrics_workspace_bytes(*a, int(fs), lpc_order, which), lib.ssr_quality_metrics,
                               (int(fs), lpc_order, which), device, deferred)


# ---- anti-wrapping phase distances: instantaneous phase, group delay, instantaneous angular frequency ---------------------------
PHASE_N_FFTS = (256, 512, 1024, 2048)


def check_phase_frames(n_fft, hop):
    """(n_fft, hop) as ints (hop None: n_fft // 4), or ValueError: n_fft one of PHASE_N_FFTS, 1 <= hop <= n_fft (the C ABI's own
    check)."""
    ints = (int, np.integer)
    if isinstance(n_fft, bool) or not isinstance(n_fft, ints) or int(n_fft) not in PHASE_N_FFTS:
        raise ValueError("n_fft must be one of %s" % (PHASE_N_FFTS,))
    hop = int(n_fft) // 4 if hop is None else hop
    if isinstance(hop, bool) or not isinstance(hop, ints) or not 1 <= int(hop) <= int(n_fft):
        raise ValueError("hop must be None (n_fft // 4) or an integer in [1, n_fft]")
    return int(n_fft), int(hop)


def phase_metrics(tgt_list, est_list, tgt_index, n_fft=1024, hop=None, band_bins=None, which=7, device=None, deferred=False):
    """Anti-wrapping phase distances of estimate e against target tgt_index[e] (ssr_phase_metrics): waveforms (float32
    or float64, each estimate as long as its target; a list holding both dtypes is widened to float64) -> [n_est, n_out] float64 in
    radians, columns in bit order of `which` (1 phase_ip, 2 phase_gd, 4 phase_iaf).  n_fft: 256, 512, 1024 or 2048; hop: None =
    n_fft // 4; band_bins: None = every bin, or (k_lo, k_hi) with 0 <= k_lo <= k_hi <= n_fft // 2, the bins scored.  Device views
    of one buffer are read where they lie.  deferred: a Pending."""
    which = int(which)
    if not 1 <= which <= 7:
        raise ValueError("which must be a non-empty combination of 1 (phase_ip), 2 (phase_gd) and 4 (phase_iaf)")
    n_fft, hop = check_phase_frames(n_fft, hop)
    k_lo, k_hi = (0, n_fft // 2) if band_bins is None else (int(band_bins[0]), int(band_bins[1]))
    if not 0 <= k_lo <= k_hi <= n_fft // 2:
        raise ValueError("band_bins must satisfy 0 <= k_lo <= k_hi <= n_fft // 2")
    lib = _lib.load()
    return _pair_index_metrics(tgt_list, est_list, tgt_index, bin(which).count("1"), _placed_where_they_lie,
                               lambda *a: lib.ssr_phase_metrics_workspace_bytes(*a, n_fft, hop, which), lib.ssr_phase_metrics,
                               (n_fft, hop, k_lo, k_hi, which), device, deferred)


# ---- multi-resolution STFT distance: spectral convergence and log-magnitude distance per resolution, and their means -----------
MRSTFT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))      # Parallel WaveGAN's (n_fft, hop, win), in samples
MRSTFT_EPS = 1e-7


def check_mrstft_resolutions(resolutions):
    """((n_fft, hop, win), ...) as a tuple of int triples (None: MRSTFT_RESOLUTIONS), or ValueError: 1 to 8 resolutions, n_fft one
    of PHASE_N_FFTS, 1 <= hop <= n_fft, 2 <= win <= n_fft (the C ABI's own check)."""
    if resolutions is None:
        return MRSTFT_RESOLUTIONS
    ints = (int, np.integer)
    if not isinstance(resolutions, (tuple, list)) or not 1 <= len(resolutions) <= _lib.MRSTFT_MAX_RES:
        raise ValueError("resolutions must be None or 1 to %d (n_fft, hop, win) triples" % _lib.MRSTFT_MAX_RES)
    out = []
    for res in resolutions:
        if not isinstance(res, (tuple, list)) or len(res) != 3 or any(isinstance(v, bool) or not isinstance(v, ints) for v in res):
            raise ValueError("a resolution is a triple of integers (n_fft, hop, win)")
        n_fft, hop, win = (int(v) for v in res)
        if n_fft not in PHASE_N_FFTS:
            raise ValueError("n_fft must be one of %s" % (PHASE_N_FFTS,))
        if not 1 <= hop <= n_fft:
            raise ValueError("hop must be in [1, n_fft]")
        if not 2 <= win <= n_fft:
            raise ValueError("win must be in [2, n_fft]")
        out.append((n_fft, hop, win))
    return tuple(out)


def check_mrstft_eps(eps):
    """eps as a float, or ValueError: finite and > 0."""
    return float(_number_in(eps, 0.0, math.inf, True, True, "eps must be a finite number > 0"))


def mrstft_metrics(tgt_list, est_list, tgt_index, resolutions=None, band_bins=None, eps=MRSTFT_EPS, device=None, deferred=False):
    """Multi-resolution STFT distance of estimate e against target tgt_index[e] (ssr_mrstft_metrics): waveforms (float32
    or float64, each estimate as long as its target; a list holding both dtypes is widened to float64) -> [n_est, n_res + 1, 2]
    float64: (spectral convergence, log-magnitude distance) per resolution, and their means over the resolutions in the last row.
    resolutions: None = MRSTFT_RESOLUTIONS, or up to 8 (n_fft, hop, win) in samples; band_bins: None = every bin, or one (k_lo, k_hi)
    or None per resolution, the bins scored.  Device views of one buffer are read where they lie.  deferred: a function that
    returns the array."""
    res = check_mrstft_resolutions(resolutions)
    eps = check_mrstft_eps(eps)
    bands = [None] * len(res) if band_bins is None else list(band_bins)
    if len(bands) != len(res):
        raise ValueError("one band per resolution")
    bins = [(0, n // 2) if b is None else (int(b[0]), int(b[1])) for (n, _, _), b in zip(res, bands)]
    if any(not 0 <= lo <= hi <= n // 2 for (n, _, _), (lo, hi) in zip(res, bins)):
        raise ValueError("band_bins must satisfy 0 <= k_lo <= k_hi <= n_fft // 2")
    tab = np.ascontiguousarray(np.array([[n, h, w, lo, hi] for (n, h, w), (lo, hi) in zip(res, bins)], np.int32).T)
    ptr = [tab[j].ctypes.data_as(C.c_void_p) for j in range(5)]
    lib = _lib.load()
    R = len(res)
    rows = _pair_index_metrics(tgt_list, est_list, tgt_index, 2 * (R + 1), _placed_where_they_lie,
                               lambda *a: lib.ssr_mrstft_workspace_bytes(*a, R, *ptr[:3]), lib.ssr_mrstft_metrics,
                               (R, *ptr, eps), device, deferred)
    if deferred:
        return lambda: rows().reshape(-1, R + 1, 2)
    return rows.reshape(-1, R + 1, 2)


# ---- filter-invariant SDR: BSS Eval's SDR with a causal FIR filter of the target as the allowed distortion ---------------------
BSS_TAPS = _lib.BSS_MAX_TAPS     # mir_eval's flen


def check_bss_taps(taps):
    """taps as an int, or ValueError: an integer in [1, 512] (the C ABI's own check)."""
    if isinstance(taps, bool) or not isinstance(taps, (int, np.integer)) or not 1 <= int(taps) <= _lib.BSS_MAX_TAPS:
        raise ValueError("taps must be an integer in [1, %d]" % _lib.BSS_MAX_TAPS)
    return int(taps)


def bss_sdr(tgt_list, est_list, tgt_index, taps=BSS_TAPS, return_filter=False, device=None, deferred=False):
    """Filter-invariant SDR of estimate e against target tgt_index[e] (ssr_bss_sdr): waveforms (float32 or float64, each
    estimate as long as its target; a list holding both dtypes is widened to float64) -> [n_est, 2] float64, columns sdr (dB) and
    sdr_lag (the tap of the largest filter coefficient, in samples); return_filter: (that, the filters [n_est, taps]).  Device views
    of one buffer are read where they lie; pairs next to each other that name one target compute its autocorrelation once.
    deferred: a Pending (return_filter: a pair of them)."""
    taps = check_bss_taps(taps)
    lib = _lib.load()
    filt = None
    if return_filter:
        dev = torch.device(device) if device is not None else default_device()
        filt = torch.empty((len(est_list), taps), dtype=torch.float64, device=dev)
    fp = _vp(filt)

    def entry(*a):      # the filters go between `out` and the workspace
        return lib.ssr_bss_sdr(*a[:-3], fp, *a[-3:])
    rows = _pair_index_metrics(tgt_list, est_list, tgt_index, 2, _placed_where_they_lie,
                               lambda *a: lib.ssr_bss_sdr_workspace_bytes(*a, taps), entry, (taps,), device, deferred)
    if not return_filter:
        return rows
    with torch.cuda.device(filt.device):
        return (rows, Pending(filt)) if deferred else (rows, filt.cpu().numpy())


# ---- magnitude-squared coherence: Welch-averaged MSC per bin, and per band its mean, the coherence SDR and the coherent bins ------
COHERENCE_THRESHOLD = 0.5


def check_coherence_frames(n_fft, hop):
    """(n_fft, hop) as ints (hop None: n_fft // 2), or ValueError: n_fft one of PHASE_N_FFTS, 1 <= hop <= n_fft (the C ABI's own
    check)."""
    ints = (int, np.integer)
    if isinstance(n_fft, bool) or not isinstance(n_fft, ints) or int(n_fft) not in PHASE_N_FFTS:
        raise ValueError("n_fft must be one of %s" % (PHASE_N_FFTS,))
    hop = int(n_fft) // 2 if hop is None else hop
    if isinstance(hop, bool) or not isinstance(hop, ints) or not 1 <= int(hop) <= int(n_fft):
        raise ValueError("hop must be None (n_fft // 2) or an integer in [1, n_fft]")
    return int(n_fft), int(hop)


def check_coherence_threshold(thr):
    """thr as a float, or ValueError: a number in (0, 1] (the C ABI's own check)."""
    return float(_number_in(thr, 0.0, 1.0, True, False, "threshold must be a number in (0, 1]"))


def coherence_metrics(tgt_list, est_list, tgt_index, n_fft=1024, hop=None, bands=None, thr=COHERENCE_THRESHOLD, return_spectrum=False,
                      device=None, deferred=False):
    """Magnitude-squared coherence of estimate e against target tgt_index[e] (ssr_coherence): waveforms (float32 or
    float64, each estimate as long as its target; a list holding both dtypes is widened to float64) -> [n_est, n_bands, 3] float64,
    (msc, coh_sdr in dB, coh_bins) per band; return_spectrum: (that, the per-bin coherence [n_est, n_fft // 2 + 1]).  n_fft: 256,
    512, 1024 or 2048; hop: None = n_fft // 2; bands: None = every bin, a list of up to 8 inclusive (lo, hi) bin pairs for every
    estimate, or one such list per estimate ([n_est][n_bands][2]); lo > hi is the empty band (NaN), otherwise 0 <= lo <= hi <=
    n_fft // 2; thr: a bin counts into coh_bins where its coherence is >= thr.  Fewer than two segments: NaN.  Device views of one
    buffer are read where they lie.  deferred: a function that returns the array (return_spectrum: the pair)."""
    n_fft, hop = check_coherence_frames(n_fft, hop)
    thr = check_coherence_threshold(thr)
    n_e, nb = len(est_list), n_fft // 2 + 1
    tab = np.asarray([(0, n_fft // 2)] if bands is None else bands)
    if tab.ndim == 2:
        tab = np.broadcast_to(tab, (n_e,) + tab.shape)
    if tab.ndim != 3 or tab.shape[0] != n_e or tab.shape[2] != 2 or not 1 <= tab.shape[1] <= _lib.MAX_BANDS or tab.dtype.kind not in "iu":
        raise ValueError("bands must be None, 1 to %d integer (lo, hi) pairs, or one such list per estimate" % _lib.MAX_BANDS)
    if np.any((tab[..., 0] <= tab[..., 1]) & ((tab[..., 0] < 0) | (tab[..., 1] > n_fft // 2))):
        raise ValueError("bands must be empty (lo > hi) or satisfy 0 <= lo <= hi <= n_fft // 2")
    tab = np.ascontiguousarray(tab, dtype=np.int32)                  # read by the library when the call is queued
    B_ = tab.shape[1]
    lib = _lib.load()
    spec = None
    if return_spectrum:
        dev = torch.device(device) if device is not None else default_device()
        spec = torch.empty((n_e, nb), dtype=torch.float64, device=dev)
    sp = _vp(spec)

    def entry(*a):      # the spectrum goes between `out` and the workspace
        return lib.ssr_coherence(*a[:-3], sp, *a[-3:])
    rows = _pair_index_metrics(tgt_list, est_list, tgt_index, 3 * B_, _placed_where_they_lie,
                               lambda *a: lib.ssr_coherence_workspace_bytes(*a, n_fft, hop, B_), entry,
                               (n_fft, hop, B_, tab.ctypes.data_as(C.c_void_p), thr), device, deferred)
    shaped = (lambda: rows().reshape(-1, B_, 3)) if deferred else rows.reshape(-1, B_, 3)
    if not return_spectrum:
        return shaped
    with torch.cuda.device(spec.device):
        return (shaped, Pending(spec)) if deferred else (shaped, spec.cpu().numpy())


# ---- loudness: BS.1770-4 integrated loudness, momentary / short-term maxima, loudness range, sample and true peak of ONE signal ----
LOUDNESS_RATES = (8000, 192000)          # SSR_LOUD_MIN_RATE, SSR_LOUD_MAX_RATE
LOUDNESS_MAX_SUB_BLOCKS = 6144           # SSR_LOUD_MAX_SUB: sub-blocks of 100 ms per signal
LOUDNESS_COLUMNS = 6


def check_loudness_rate(rate):
    """rate as an int, or ValueError: a whole number of Hz in LOUDNESS_RATES (the C ABI's own check)."""
    ok = _is_number(rate) and float(rate) == int(rate)
    if not ok or not LOUDNESS_RATES[0] <= int(rate) <= LOUDNESS_RATES[1]:
        raise ValueError("the loudness family needs an integer rate in [%d, %d] Hz" % LOUDNESS_RATES)
    return int(rate)


def loudness_sub_len(rate):
    """Samples per 100 ms sub-block at `rate`: round(rate / 10), halves up."""
    return (int(rate) + 5) // 10


def loudness_metrics(sig_list, rate, return_blocks=False, device=None, deferred=False):
    """The six EBU R128 meter quantities of every signal (ssr_loudness): waveforms (float32 or float64; a list holding
    both dtypes is widened to float64) at the integer `rate` -> [n, 6] float64, columns lufs, lra, lufs_m_max, lufs_s_max,
    peak_db, true_peak_db (NaN where a block set is empty; both peaks NaN for digital silence).  return_blocks: (that, a list of
    n float64 arrays, the K-weighted energies E[s] of the signals' 100 ms sub-blocks).  Device views of one buffer are read where
    they lie.  A signal of more than LOUDNESS_MAX_SUB_BLOCKS sub-blocks is refused.  deferred: a function that returns the array
    (return_blocks: the pair)."""
    rate = check_loudness_rate(rate)
    sigs = list(sig_list)
    n = len(sigs)
    lib, dev = _gpu_call(device)
    with torch.cuda.device(dev):
        out = torch.empty((n, LOUDNESS_COLUMNS), dtype=torch.float64, device=dev)
        blocks, counts = None, None
        if n:
            (data, f64, off), lens = _placed_signals(sigs, dev)
            counts = lens // loudness_sub_len(rate)
            if counts.max() > LOUDNESS_MAX_SUB_BLOCKS:
                raise ValueError("a signal may hold at most %d sub-blocks of 100 ms" % LOUDNESS_MAX_SUB_BLOCKS)
            lens32 = lens.astype(np.int32)
            ws_bytes = int(lib.ssr_loudness_workspace_bytes(lens32.ctypes.data_as(C.c_void_p), n, rate))
            ws = _workspace(ws_bytes, dev)
            lens_h = _host_i32(lens32, dev)
            boff = None
            if return_blocks:
                boff = np.ascontiguousarray(_offsets(counts), dtype=np.int64)            # read by the library when the call is queued
                blocks = torch.empty(int(counts.sum()), dtype=torch.float64, device=dev)
            _lib.check(lib.ssr_loudness(_vp(data), int(f64), _vp(off), _vp(lens_h), n, rate, _vp(out),
                                        boff.ctypes.data_as(C.c_void_p) if return_blocks else None, _vp(blocks), _vp(ws), ws_bytes,
                                        _stream()))
        rows = Pending(out) if deferred else out.cpu().numpy()
        if not return_blocks:
            return rows
        if blocks is None or blocks.numel() == 0:
            empty = [np.empty(0) for _ in range(n)]
            return (rows, (lambda: empty)) if deferred else (rows, empty)
        edges = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        split = lambda flat: [np.array(flat[edges[i]:edges[i + 1]]) for i in range(n)]      # noqa: E731
        flat = Pending(blocks) if deferred else blocks.cpu().numpy()
        return (rows, (lambda: split(flat()))) if deferred else (rows, split(flat))


# ---- spectrum: rolloff bandwidth, spectral edge, centroid, HF level and LTAS distance from the long-term average spectrum -----------
SPECTRUM_ROLLOFF = 0.97                  # the reference's BasicTestee._find_cutoff threshold
SPECTRUM_DROP_DB = 60.0
SPECTRUM_MAX_BANDS = _lib.SPECTRUM_MAX_BANDS
SPECTRUM_SIG_COLUMNS, SPECTRUM_PAIR_COLUMNS = 3, 8      # SSR_SPECTRUM_SIG_COLS, SSR_SPECTRUM_PAIR_COLS


def check_spectrum_rolloff(rho):
    """rho as a float, or ValueError: a number in (0, 1) (the C ABI's own check)."""
    return float(_number_in(rho, 0.0, 1.0, True, True, "rolloff must be a number in (0, 1)"))


def check_spectrum_drop(drop_db):
    """drop_db as a float, or ValueError: a number in (0, 150] (the C ABI's own check)."""
    return float(_number_in(drop_db, 0.0, 150.0, True, False, "drop_db must be a number in (0, 150]"))


def spectrum_metrics(tgt_list, est_list, tgt_index, n_fft=2048, hop=None, band_bins=None, rolloff=SPECTRUM_ROLLOFF,
                     drop_db=SPECTRUM_DROP_DB, bands=None, split_bins=None, return_ltas=False, device=None, deferred=False):
    """The spectrum family (ssr_spectrum) on the signals tgt_list + est_list, estimate e belonging to target tgt_index[e]
    and as long as it (float32 or float64 waveforms; a list holding both dtypes is widened to float64) -> (sig [n_tgt + n_est, 3]
    float64: rolloff bin, edge bin, centroid in bins; pair [n_est, 8] float64: hf_db of the estimate and of the target, the rolloff /
    edge / centroid differences in bins, hf_diff, ltas_dist, ltas_max); return_ltas: also c P / K per bin, [n_tgt + n_est,
    n_fft // 2 + 1].  est_list = [] measures the targets alone.  n_fft: 256, 512, 1024 or 2048; hop: None = n_fft // 2; band_bins:
    None = every bin, or (lo, hi) - lo > hi is the empty band (NaN); bands: None = one analysis band over every bin, or up to 40
    disjoint ascending inclusive (lo, hi) bin pairs; split_bins: None, or per estimate the first bin of the upper part (-1: none).
    Device views of one buffer are read where they lie.  deferred: a function that returns the tuple."""
    n_fft, hop = check_coherence_frames(n_fft, hop)                 # (§20's framing)
    rho, drop = check_spectrum_rolloff(rolloff), check_spectrum_drop(drop_db)
    lo, hi = (0, n_fft // 2) if band_bins is None else (int(band_bins[0]), int(band_bins[1]))
    if lo <= hi and (lo < 0 or hi > n_fft // 2):
        raise ValueError("band_bins must be empty (lo > hi) or satisfy 0 <= lo <= hi <= n_fft // 2")
    tab = np.asarray([(0, n_fft // 2)] if bands is None else bands)
    if tab.ndim != 2 or tab.shape[1] != 2 or not 1 <= tab.shape[0] <= SPECTRUM_MAX_BANDS or tab.dtype.kind not in "iu":
        raise ValueError("bands must be None or 1 to %d integer (lo, hi) pairs" % SPECTRUM_MAX_BANDS)
    if np.any(tab[:, 0] < 0) or np.any(tab[:, 0] > tab[:, 1]) or np.any(tab[:, 1] > n_fft // 2) or np.any(tab[1:, 0] <= tab[:-1, 1]):
        raise ValueError("bands must be disjoint ascending ranges with 0 <= lo <= hi <= n_fft // 2")
    tab = np.ascontiguousarray(tab, dtype=np.int32)                      # read by the library when the call is queued
    tgts, ests, idx = _signal_pair_index(tgt_list, est_list, tgt_index)
    n_t, n_e, nb = len(tgts), len(ests), n_fft // 2 + 1
    sp = _split_array(split_bins, n_e, lambda s: s.min() >= -1, "split_bins must hold one bin >= 0, or -1 for none, per estimate")
    lib, dev = _gpu_call(device)
    with torch.cuda.device(dev):
        sig = torch.empty((n_t + n_e, SPECTRUM_SIG_COLUMNS), dtype=torch.float64, device=dev)
        pair = torch.empty((n_e, SPECTRUM_PAIR_COLUMNS), dtype=torch.float64, device=dev)
        ltas = torch.empty((n_t + n_e, nb), dtype=torch.float64, device=dev) if return_ltas else None
        if n_t:
            tgt_side, est_side, tl = _signal_pair_place(tgts, ests, idx, dev)
            lens = tl.astype(np.int32)
            B_ = tab.shape[0]
            ws_bytes = int(lib.ssr_spectrum_workspace_bytes(lens.ctypes.data_as(C.c_void_p), n_t, idx.ctypes.data_as(C.c_void_p), n_e,
                                                            n_fft, hop, B_))
            ws = _workspace(ws_bytes, dev)
            lens_h, idx_h, sp_h = _host_i32(lens, dev), _host_i32(idx, dev), _host_i32(sp, dev)
            _lib.check(lib.ssr_spectrum(*_args(tgt_side), _vp(lens_h), n_t, *_args(est_side), _vp(idx_h) if n_e else None, n_e, n_fft, hop,
                                        lo, hi, rho, drop, B_, tab.ctypes.data_as(C.c_void_p), _vp(sp_h) if n_e else None, _vp(sig),
                                        _vp(pair) if n_e else None, _vp(ltas), _vp(ws), ws_bytes, _stream()))
        return _collected([_take(sig), _take(pair)] + ([_take(ltas)] if return_ltas else []), deferred)


# ---- auditory: neurogram similarity (NSIM) of gammatone spectrograms --------------------------------------------------------------
AUDITORY_BANDS = (3, 64)                 # SSR_AUDITORY_MIN_BANDS, SSR_AUDITORY_MAX_BANDS
AUDITORY_N_BANDS = 32
AUDITORY_RANGE_DB = 60.0
AUDITORY_MAX_BLOCKS = 65536              # SSR_AUDITORY_MAX_BLOCKS: hop-blocks per signal
AUDITORY_PAIR_COLUMNS = 3                # SSR_AUDITORY_PAIR_COLS
_GAMMATONE_A = math.pi * 720.0 * 2.0 ** -6 / 36.0      # a_gamma of order 4: pi 6! 2^-6 / (3!)^2


def check_auditory_bands(n_bands):
    """n_bands as an int, or ValueError: an integer in AUDITORY_BANDS (the C ABI's own check)."""
    if isinstance(n_bands, bool) or not isinstance(n_bands, (int, np.integer)) or not AUDITORY_BANDS[0] <= int(n_bands) <= AUDITORY_BANDS[1]:
        raise ValueError("n_bands must be an integer in [%d, %d]" % AUDITORY_BANDS)
    return int(n_bands)


def check_auditory_range(range_db):
    """range_db as a float, or ValueError: a number in (0, 150] (the C ABI's own check)."""
    return float(_number_in(range_db, 0.0, 150.0, True, False, "range_db must be a number in (0, 150]"))


def auditory_hop(fs):
    """Samples per 10 ms block at `fs`: round(fs / 100), halves up; the image's window is two of them."""
    _number_in(fs, 50.0, math.inf, False, True, "the auditory family needs a rate of at least 50 Hz")
    return int(math.floor(float(fs) / 100.0 + 0.5))


def gammatone_design(fs, n_bands=AUDITORY_N_BANDS, band=None):
    """Hohmann's complex all-pole gammatone filterbank of order 4 at rate fs -> (f_c [n_bands] in Hz, coef [n_bands, 3]
    float64 = Re a, Im a, g): centres equally spaced on the ERB-number scale 21.4 log10(1 + 0.00437 f) from band[0] to band[1]
    inclusive (None: 50 Hz to 0.45 fs); b = ERBN(f_c) / a_gamma, lambda = exp(-2 pi b / fs), a = lambda exp(i 2 pi f_c / fs),
    g = 2 (1 - lambda)^4, so that |H(f_c)| = 2.  ValueError unless 3 <= n_bands <= 64 and 0 < lo < hi < fs / 2."""
    n_bands = check_auditory_bands(n_bands)
    auditory_hop(fs)
    fs = float(fs)
    if band is None:
        band = (50.0, 0.45 * fs)
    ok = isinstance(band, (tuple, list)) and len(band) == 2 and all(_is_number(v) for v in band)
    if not ok or not 0.0 < float(band[0]) < float(band[1]) < fs / 2.0:
        raise ValueError("band must be None or (lo_hz, hi_hz) with 0 < lo_hz < hi_hz < fs / 2")
    scale = lambda f: 21.4 * math.log10(1.0 + 0.00437 * f)      # noqa: E731
    e = np.linspace(scale(float(band[0])), scale(float(band[1])), n_bands)
    fc = (10.0 ** (e / 21.4) - 1.0) / 0.00437
    lam = np.exp(-2.0 * np.pi * (24.7 * (1.0 + 0.00437 * fc) / _GAMMATONE_A) / fs)
    coef = np.stack([lam * np.cos(2.0 * np.pi * fc / fs), lam * np.sin(2.0 * np.pi * fc / fs), 2.0 * (1.0 - lam) ** 4], axis=1)
    return fc, np.ascontiguousarray(coef, dtype=np.float64)


def auditory_metrics(tgt_list, est_list, tgt_index, fs, n_bands=AUDITORY_N_BANDS, band=None, range_db=AUDITORY_RANGE_DB, match_level=True,
                     split_bands=None, return_bands=False, return_images=False, hop=None, device=None, deferred=False):
    """The auditory family (ssr_auditory) on the signals tgt_list + est_list at rate fs, estimate e belonging to target
    tgt_index[e] and as long as it (float32 or float64 waveforms; a list holding both dtypes is widened to float64) -> (pair [n_est, 3]
    float64: nsim, nsim_hf, nsim_lf; bands [n_est, n_bands]: the mean NSIM of every interior band, NaN in the two edge bands, or None
    without return_bands; images: a list of the n_tgt + n_est dB images [T, n_bands] - an estimate's level matched and on its target's
    floor - or None without return_images).  est_list = [] with return_images yields the targets' images.  split_bands: None, or per
    estimate the first interior band of its upper part (n_bands - 1: none above; -1: no split); hop: None = auditory_hop(fs) (the
    definition's 10 ms), or the samples per block.  A signal of more than AUDITORY_MAX_BLOCKS blocks is refused.  Device views of
    one buffer are read where they lie.  The library keeps a small table (about 120 n_bands bytes) per distinct (fs, n_bands, band,
    hop) for the life of the process: a sweep over thousands of designs pays that memory.  deferred: a function that returns the
    tuple."""
    _, coef = gammatone_design(fs, n_bands, band)
    C_ = coef.shape[0]
    rng_db = check_auditory_range(range_db)
    if not isinstance(match_level, (bool, np.bool_)):
        raise ValueError("match_level must be True or False")
    hop = auditory_hop(fs) if hop is None else hop
    if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or int(hop) < 1:
        raise ValueError("hop must be None or an integer >= 1")
    hop = int(hop)
    tgts, ests, idx = _signal_pair_index(tgt_list, est_list, tgt_index)
    n_t, n_e = len(tgts), len(ests)
    sp = _split_array(split_bands, n_e, lambda s: s.min() >= -1 and s.max() <= C_ - 1 and not np.any(s == 0),
                      "split_bands must hold -1 or a band in [1, n_bands - 1] per estimate")
    lib, dev = _gpu_call(device)
    with torch.cuda.device(dev):
        pair = torch.empty((n_e, AUDITORY_PAIR_COLUMNS), dtype=torch.float64, device=dev)
        bands = torch.empty((n_e, C_), dtype=torch.float64, device=dev) if return_bands else None
        images, rows = None, np.zeros(0, np.int64)
        if n_t:
            tgt_side, est_side, tl = _signal_pair_place(tgts, ests, idx, dev)
            rows = np.maximum(_hop_blocks(tl, hop, AUDITORY_MAX_BLOCKS) - 1, 0).astype(np.int64)
            rows = np.concatenate([rows, rows[idx]])
            if return_images:
                images = torch.empty((int(rows.sum()), C_), dtype=torch.float64, device=dev)
            lens = tl.astype(np.int32)
            ws_bytes = int(lib.ssr_auditory_workspace_bytes(lens.ctypes.data_as(C.c_void_p), n_t, idx.ctypes.data_as(C.c_void_p), n_e, hop, C_))
            ws = _workspace(ws_bytes, dev)
            lens_h, idx_h, sp_h = _host_i32(lens, dev), _host_i32(idx, dev), _host_i32(sp, dev)
            # (coef is read by the library before the call returns: its table of the call is built on the host)
            _lib.check(lib.ssr_auditory(*_args(tgt_side), _vp(lens_h), n_t, *_args(est_side), _vp(idx_h) if n_e else None, n_e, hop, C_,
                                        coef.ctypes.data_as(C.c_void_p), rng_db, int(bool(match_level)), _vp(sp_h) if n_e else None,
                                        _vp(pair) if n_e else None, _vp(bands), _vp(images), _vp(ws), ws_bytes, _stream()))
        got = [_take(pair), _take(bands) if return_bands else (lambda: None)]
        if return_images:
            edges = np.concatenate(([0], np.cumsum(rows))).astype(np.int64)
            flat = _take(images) if images is not None else (lambda: np.empty((0, C_)))

            def cut():
                a = flat()
                return [np.array(a[edges[i]:edges[i + 1]]) for i in range(len(rows))]
            got.append(cut)
        else:
            got.append(lambda: None)
        return _collected(got, deferred)


# ---- modulation: SRMR and the modulation-spectrum distance on §23's filterbank ------------------------------------------------------
MODULATION_BANDS = 8                     # SSR_MODULATION_BANDS: modulation bands per gammatone band
MODULATION_Q = 2.0
MODULATION_ENV_RATE = 1600               # Hz, the envelope rate aimed at
MODULATION_ENV_RATES = (800, 6400)
MODULATION_RANGE_DB = 60.0
MODULATION_MAX_BLOCKS = 65536            # SSR_MODULATION_MAX_BLOCKS: envelope samples per signal
MODULATION_MAX_STEP = 1024               # SSR_MODULATION_MAX_STEP
MODULATION_SIGNAL_COLUMNS = 4            # SSR_MODULATION_SIGNAL_COLS: srmr, K*, c90, sum Ebar
MODULATION_PAIR_COLUMNS = 4              # SSR_MODULATION_PAIR_COLS: srmr_diff, mod_dist, mod_dist_hf, mod_dist_lf
MODULATION_WORKSPACE_CAP = 1 << 30       # bytes of workspace one ssr_modulation call may ask for: larger batches are split


def check_modulation_env_rate(env_rate):
    """env_rate as it is, or ValueError: a number in MODULATION_ENV_RATES (Hz)."""
    return _number_in(env_rate, *MODULATION_ENV_RATES, False, False, "env_rate must be a number in [%d, %d] Hz" % MODULATION_ENV_RATES)


def check_modulation_range(range_db):
    """range_db as a float, or ValueError: a number in (0, 150] (the C ABI's own check)."""
    return check_auditory_range(range_db)


def check_modulation_kstar(kstar):
    """kstar as it is, or ValueError: None (the adaptive table) or an integer in [5, 8] (the C ABI's own check)."""
    if kstar is not None and (isinstance(kstar, bool) or not isinstance(kstar, (int, np.integer)) or not 5 <= int(kstar) <= MODULATION_BANDS):
        raise ValueError("kstar must be None or an integer in [5, %d]" % MODULATION_BANDS)
    return kstar if kstar is None else int(kstar)


def modulation_hop(fs, env_rate=MODULATION_ENV_RATE):
    """hop_e = max(1, fs // env_rate): the samples of `fs` per envelope sample; the envelope's rate is fs / hop_e."""
    auditory_hop(fs)
    return max(1, int(float(fs) // float(check_modulation_env_rate(env_rate))))


def modulation_design(fs, hop_e, n_bands=AUDITORY_N_BANDS, band=None, kstar=None):
    """The two filterbanks of the modulation family at rate fs -> (f_c [n_bands] in Hz, coef [n_bands, 3]: gammatone_design's,
    mod [8, 5] float64 = (b0, b1, b2, a1, a2) of the modulation band-passes at the envelope rate fe = fs / hop_e, S: the frame step in
    envelope samples, kstar_table [n_bands] int32).  Modulation band k: centre f_k = 4 * 32^(k / 7) Hz, Q = 2, the bilinear (RBJ)
    band-pass of unit peak gain: w0 = 2 pi f_k / fe, alpha = sin w0 / (2 Q), b = (alpha, 0, -alpha) / (1 + alpha),
    a = (1, -2 cos w0 / (1 + alpha), (1 - alpha) / (1 + alpha)).  S = round(0.064 fe) (frames of 4 S).  kstar_table[c]: `kstar` where
    it is given, else 4 + the number of k in 4 .. 7 whose lower -3 dB edge f_k (sqrt(1 + 1 / (4 Q^2)) - 1 / (2 Q)) lies below
    ERB(f_c[c]) = 24.7 (1 + 0.00437 f_c[c]), at least 5.  ValueError unless fe >= 400 Hz and S <= MODULATION_MAX_STEP."""
    fc, coef = gammatone_design(fs, n_bands, band)
    kstar = check_modulation_kstar(kstar)
    if isinstance(hop_e, bool) or not isinstance(hop_e, (int, np.integer)) or int(hop_e) < 1:
        raise ValueError("hop_e must be an integer >= 1")
    fe = float(fs) / int(hop_e)
    S = int(math.floor(0.064 * fe + 0.5))
    if fe < 400.0 or S > MODULATION_MAX_STEP:
        raise ValueError("the modulation family needs an envelope rate fs / hop_e in [400, 16000] Hz")
    Q = MODULATION_Q
    fk = 4.0 * 32.0 ** (np.arange(MODULATION_BANDS) / (MODULATION_BANDS - 1.0))
    w0 = 2.0 * np.pi * fk / fe
    alpha = np.sin(w0) / (2.0 * Q)
    mod = np.stack([alpha / (1.0 + alpha), np.zeros_like(alpha), -alpha / (1.0 + alpha), -2.0 * np.cos(w0) / (1.0 + alpha),
                    (1.0 - alpha) / (1.0 + alpha)], axis=1)
    if kstar is None:
        edge = fk[4:] * (math.sqrt(1.0 + 1.0 / (4.0 * Q * Q)) - 1.0 / (2.0 * Q))
        erb = 24.7 * (1.0 + 0.00437 * fc)
        table = np.maximum(4 + np.sum(edge[None, :] < erb[:, None], axis=1), 5)
    else:
        table = np.full(len(fc), kstar)
    return fc, coef, np.ascontiguousarray(mod, dtype=np.float64), S, np.ascontiguousarray(table, dtype=np.int32)


def modulation_metrics(tgt_list, est_list, tgt_index, fs, n_bands=AUDITORY_N_BANDS, band=None, env_rate=MODULATION_ENV_RATE,
                       range_db=MODULATION_RANGE_DB, kstar=None, split_bands=None, return_spectrum=False, hop_e=None, device=None,
                       deferred=False):
    """The modulation family (ssr_modulation) on the signals tgt_list + est_list at rate fs, estimate e belonging to target
    tgt_index[e] and as long as it (float32 or float64 waveforms; a list holding both dtypes is widened to float64) -> (signal
    [n_tgt + n_est, 4] float64: srmr, K*, c90, sum Ebar of the targets, then of the estimates; pair [n_est, 4]: srmr_diff, mod_dist,
    mod_dist_hf, mod_dist_lf; spectrum [n_tgt + n_est, n_bands, 8]: Ebar, or None without return_spectrum).  est_list = [] is the
    non-intrusive call.  split_bands: None, or per estimate the first band of its upper part in [0, n_bands] (-1: no split); hop_e:
    None = modulation_hop(fs, env_rate), or the samples per envelope sample.  A signal of more than MODULATION_MAX_BLOCKS envelope
    samples is refused.  The workspace holds about 16 n_bands bytes per envelope sample; a batch that would need more than
    MODULATION_WORKSPACE_CAP bytes is split into calls of whole targets with their estimates, which changes no bit: a signal gives
    the same bits in any batch.  Device views of one buffer are read where they lie.  deferred: a function that returns the tuple."""
    rng_db = check_modulation_range(range_db)
    hop = modulation_hop(fs, env_rate) if hop_e is None else hop_e
    _, coef, mod, S, ktab = modulation_design(fs, hop, n_bands, band, kstar)
    hop = int(hop)
    C_ = coef.shape[0]
    if not isinstance(return_spectrum, (bool, np.bool_)):
        raise ValueError("return_spectrum must be True or False")
    tgts, ests, idx = _signal_pair_index(tgt_list, est_list, tgt_index)
    n_t, n_e = len(tgts), len(ests)
    sp = _split_array(split_bands, n_e, lambda s: s.min() >= -1 and s.max() <= C_, "split_bands must hold -1 or a band in [0, n_bands] per estimate")
    lib, dev = _gpu_call(device)
    parts = []                                   # (target positions, estimate positions, signal, pair, spectrum) per call
    with torch.cuda.device(dev):
        if n_t:
            tgt_side, est_side, tl = _signal_pair_place(tgts, ests, idx, dev)
            blocks = _hop_blocks(tl, hop, MODULATION_MAX_BLOCKS)
            # whole targets with their estimates, in target order, under the cap (a target that exceeds it alone is a call of its own)
            cost = (blocks + 7) // 8 * 8 * C_ * 16 * (1 + np.bincount(idx, minlength=n_t))
            cuts, acc = [0], 0
            for t in range(n_t):
                if acc and acc + cost[t] > MODULATION_WORKSPACE_CAP:
                    cuts.append(t)
                    acc = 0
                acc += int(cost[t])
            cuts.append(n_t)
            ktab_h = _host_i32(ktab, dev)
            for t0, t1 in zip(cuts[:-1], cuts[1:]):
                es = np.nonzero((idx >= t0) & (idx < t1))[0]
                g_t, g_e = t1 - t0, len(es)
                lens, gidx, gsp = tl[t0:t1].astype(np.int32), (idx[es] - t0).astype(np.int32), sp[es]
                if g_e and not np.array_equal(es, np.arange(es[0], es[0] + g_e)):
                    e_off = est_side[2][_h2d(es.astype(np.int64), dev)]
                else:
                    e_off = est_side[2][int(es[0]):int(es[0]) + g_e] if g_e else None
                sig = torch.empty((g_t + g_e, MODULATION_SIGNAL_COLUMNS), dtype=torch.float64, device=dev)
                pair = torch.empty((g_e, MODULATION_PAIR_COLUMNS), dtype=torch.float64, device=dev)
                spec = torch.empty((g_t + g_e, C_, MODULATION_BANDS), dtype=torch.float64, device=dev) if return_spectrum else None
                ws_bytes = int(lib.ssr_modulation_workspace_bytes(lens.ctypes.data_as(C.c_void_p), g_t, gidx.ctypes.data_as(C.c_void_p), g_e, hop, C_))
                ws = _workspace(ws_bytes, dev)
                lens_h, idx_h, sp_h = _host_i32(lens, dev), _host_i32(gidx, dev), _host_i32(gsp, dev)
                # (coef and mod are read by the library before the call returns: its tables of the call are built on the host)
                _lib.check(lib.ssr_modulation(_vp(tgt_side[0]), tgt_side[1], _vp(tgt_side[2][t0:t1]), _vp(lens_h), g_t,
                                              _vp(est_side[0]) if g_e else None, est_side[1], _vp(e_off), _vp(idx_h) if g_e else None, g_e,
                                              hop, C_, coef.ctypes.data_as(C.c_void_p), mod.ctypes.data_as(C.c_void_p), S, _vp(ktab_h), rng_db,
                                              _vp(sp_h) if g_e else None, _vp(sig), _vp(pair) if g_e else None, _vp(spec), _vp(ws), ws_bytes,
                                              _stream()))
                parts.append((np.arange(t0, t1), es, Pending(sig), Pending(pair) if g_e else None, Pending(spec) if return_spectrum else None))

        def collect():
            signal = np.full((n_t + n_e, MODULATION_SIGNAL_COLUMNS), np.nan)
            pair = np.full((n_e, MODULATION_PAIR_COLUMNS), np.nan)
            spectrum = np.full((n_t + n_e, C_, MODULATION_BANDS), np.nan) if return_spectrum else None
            for ts, es, sig_p, pair_p, spec_p in parts:
                where = np.concatenate([ts, n_t + es]).astype(np.int64)
                signal[where] = sig_p()
                if pair_p is not None:
                    pair[es] = pair_p()
                if spec_p is not None:
                    spectrum[where] = spec_p()
            return signal, pair, spectrum
        return collect if deferred else collect()


# ---- csii: the coherence speech intelligibility index and the fitted three-level I3 on §20's spectra -----------------
CSII_CENTRES = (150.0, 250.0, 350.0, 450.0, 570.0, 700.0, 840.0, 1000.0, 1170.0, 1370.0, 1600.0, 1850.0, 2150.0, 2500.0, 2900.0, 3400.0,
                4000.0, 4800.0, 5800.0, 7000.0, 8500.0)         # Hz: the critical bands of ANSI S3.5-1997
CSII_IMPORTANCE = (0.0103, 0.0261, 0.0419) + (0.0577,) * 14 + (0.0460, 0.0343, 0.0226, 0.0110)        # their band importance, sum 1
CSII_COLUMNS = _lib.CSII_COLUMNS         # SSR_CSII_COLUMNS: the nine values, then the segments in the four sets
CSII_SETS = 4                            # all, low, mid, high
_CSII_WEIGHTS = {}                       # (rate, n_fft, band, device index) -> the device copy of csii_design's W


def csii_default_nfft(fs):
    """The segment length at rate fs: the smallest of PHASE_N_FFTS that holds 16 ms, 2048 where none does (256 at 16 kHz, 1024 at
    44.1 and 48 kHz).  ValueError unless fs is a number above 300 Hz (the lowest critical band centre lies at 150 Hz)."""
    _number_in(fs, 300.0, math.inf, True, True, "the csii family needs a rate above 300 Hz")
    return next((n for n in PHASE_N_FFTS if n >= 0.016 * float(fs)), PHASE_N_FFTS[-1])


def check_csii_frames(fs, n_fft, hop):
    """(n_fft, hop) as ints (n_fft None: csii_default_nfft(fs); hop None: n_fft // 2), or ValueError: §20's framing."""
    return check_coherence_frames(csii_default_nfft(fs) if n_fft is None else n_fft, hop)


def csii_design(fs, n_fft, band=None):
    """The critical-band stage at rate fs on n_fft-point segments -> (f_c [n_bands] in Hz, importance [n_bands] float64
    with sum 1, W [n_bands, n_fft // 2 + 1] float64): the bands of ANSI S3.5-1997 with f_c <= fs / 2 (17 at 8 kHz, 20 at 16 kHz, all 21
    from 17 kHz) - inside band = (lo_hz, hi_hz),
    both ends included, if one is given -, their importance renormalised, and the rounded-exponential weights W_j[k] = (1 + p g)
    exp(-p g) with g = |k fs / n_fft - f_c| / f_c and p = 4 f_c / ERB(f_c), ERB = 24.7 (4.37 f_c / 1000 + 1); W_j[0] = 0.
    ValueError unless n_fft is one of PHASE_N_FFTS and at least one band is left."""
    csii_default_nfft(fs)
    n_fft, _ = check_coherence_frames(n_fft, None)
    fs = float(fs)
    ok = band is None or (isinstance(band, (tuple, list)) and len(band) == 2 and all(_is_number(v) for v in band) and
                          0.0 <= float(band[0]) <= float(band[1]))
    keep = [j for j, f in enumerate(CSII_CENTRES) if f <= fs / 2.0 and (band is None or float(band[0]) <= f <= float(band[1]))] if ok else []
    if not keep:
        raise ValueError("band must be None or (lo_hz, hi_hz) with 0 <= lo_hz <= hi_hz and a critical-band centre up to fs / 2 inside it")
    fc = np.array([CSII_CENTRES[j] for j in keep], np.float64)
    imp = np.array([CSII_IMPORTANCE[j] for j in keep], np.float64)
    imp = imp / imp.sum()
    p = 4.0 * fc / (24.7 * (4.37 * fc / 1000.0 + 1.0))
    g = np.abs(np.arange(n_fft // 2 + 1, dtype=np.float64)[None, :] * (fs / n_fft) - fc[:, None]) / fc[:, None]
    W = (1.0 + p[:, None] * g) * np.exp(-p[:, None] * g)
    W[:, 0] = 0.0
    return fc, np.ascontiguousarray(imp), np.ascontiguousarray(W)


def csii_metrics(tgt_list, est_list, tgt_index, fs, n_fft=None, hop=None, band=None, split_bands=None, return_bands=False, device=None,
                 deferred=False):
    """The coherence speech intelligibility index of estimate e against target tgt_index[e] (ssr_csii): waveforms at rate
    fs (float32 or float64, each estimate as long as its target; a list holding both dtypes is widened to float64) -> (rows [n_est,
    13] float64: csii over all segments, csii_low, csii_mid, csii_high, i3, the value above the split of the four sets in that
    order, then the segments in the four sets; bands [n_est, 4, n_bands]: the band values T_j of every set, or None without
    return_bands).  n_fft: None = csii_default_nfft(fs), or 256, 512, 1024 or 2048; hop: None = n_fft // 2; band: None or (lo_hz,
    hi_hz), the critical-band centres kept; split_bands: None, or per estimate the first band of its upper part in [0, n_bands]
    (n_bands: none above; -1: no split).  A set of fewer than two segments and a digitally silent target: NaN.  The workspace holds
    128 (n_fft / 2 + 1) bytes per chunk of 32 segments of every pair.  Device views of one buffer are read where they lie.
    deferred: a function that returns the tuple."""
    n_fft, hop = check_csii_frames(fs, n_fft, hop)
    _, imp, W = csii_design(fs, n_fft, band)
    J = imp.shape[0]
    if not isinstance(return_bands, (bool, np.bool_)):
        raise ValueError("return_bands must be True or False")
    tgts, ests, idx = _signal_pair_index(tgt_list, est_list, tgt_index)
    n_t, n_e = len(tgts), len(ests)
    sp = _split_array(split_bands, n_e, lambda s: s.min() >= -1 and s.max() <= J, "split_bands must hold -1 or a band in [0, n_bands] per estimate")
    lib, dev = _gpu_call(device)
    with torch.cuda.device(dev):
        rows = torch.empty((n_e, CSII_COLUMNS), dtype=torch.float64, device=dev)
        bands = torch.empty((n_e, CSII_SETS, J), dtype=torch.float64, device=dev) if return_bands else None
        if n_e:
            tgt_side, est_side, tl = _signal_pair_place(tgts, ests, idx, dev)
            lens = tl.astype(np.int32)
            ws_bytes = int(lib.ssr_csii_workspace_bytes(lens.ctypes.data_as(C.c_void_p), n_t, idx.ctypes.data_as(C.c_void_p), n_e, n_fft, hop, J))
            ws = _workspace(ws_bytes, dev)
            lens_h, idx_h, sp_h = _host_i32(lens, dev), _host_i32(idx, dev), _host_i32(sp, dev)
            # the weights stay on the device for the life of the process, one table (at most 172 KB) per (rate, n_fft, band, device);
            # the importance is read by the library out of page-locked memory, like the three int32 arrays: no copy waits for the stream
            key = (float(fs), n_fft, None if band is None else (float(band[0]), float(band[1])), torch.cuda.current_device())
            w_dev = _CSII_WEIGHTS.get(key)
            if w_dev is None:
                w_dev = _CSII_WEIGHTS[key] = _h2d(W, dev)
            imp_h = _DescRing.get(torch.cuda.current_device()).stage(imp, dev)
            _lib.check(lib.ssr_csii(*_args(tgt_side), _vp(lens_h), n_t, *_args(est_side), _vp(idx_h), n_e, n_fft, hop, J, _vp(w_dev),
                                    _vp(imp_h), _vp(sp_h), _vp(rows), _vp(bands), _vp(ws), ws_bytes, _stream()))
        return _collected([_take(rows), _take(bands) if return_bands else (lambda: None)], deferred)


# ---- nmr: the noise-to-mask ratio on the FFT ear model of BS.1387, restated ---------------------------------------------
NMR_COLUMNS = _lib.NMR_COLUMNS           # SSR_NMR_COLUMNS: nmr, nmr_seg, rdf, nmr_hf, nmr_lf, frames
NMR_LEVEL_DB = 92.0                      # the level of a full-scale sine in dB SPL
NMR_DZ = 0.25                            # band width in Bark
_NMR_DESIGNS = {}                        # (rate, n_fft, level_db) -> nmr_design's dict
_NMR_WEIGHTS = {}                        # (rate, n_fft, level_db, device index) -> the device copy of its weights


def nmr_default_nfft(fs):
    """The frame length at rate fs: the smallest of PHASE_N_FFTS that holds 32 ms, 2048 where none does (256 at 8 kHz, 512 at 16 kHz,
    1024 at 24 and 32 kHz, 2048 at 44.1 and 48 kHz).  ValueError unless fs is a number from 8 to 192 kHz."""
    _number_in(fs, 8000.0, 192000.0, False, False, "the nmr family needs a rate from 8000 to 192000 Hz")
    return next((n for n in PHASE_N_FFTS if n >= 0.032 * float(fs)), PHASE_N_FFTS[-1])


def check_nmr_options(fs, n_fft, level_db):
    """(n_fft as an int - None: nmr_default_nfft(fs) -, level_db as a float), or ValueError."""
    default = nmr_default_nfft(fs)
    n_fft, _ = check_coherence_frames(default if n_fft is None else n_fft, None)
    _number_in(level_db, 0.0, 200.0, False, False, "level_db must be a number in [0, 200]")
    return n_fft, float(level_db)


def nmr_design(fs, n_fft=None, level_db=NMR_LEVEL_DB):
    """Every table of DESIGN §28 at rate fs for n_fft-point frames, cached per (fs, n_fft, level_db) -> a dict: 'n_fft', 'fc' [Nc] the
    band centres in Hz, 'weights' [n_fft // 2 + 1] = G W2 (level and ear weighting), 'bins' [Nc, 2] int32 = (k_lo, k_hi), 'table' [Nc,
    8] = (u_lo, u_hi, Ein, c_up, ad, 1 / Bs, a, mgain) - the arrays ssr_nmr takes - and 'mask_db' [Nc], the offset m_i."""
    n_fft, level_db = check_nmr_options(fs, n_fft, level_db)
    fs = float(fs)
    key = (fs, n_fft, level_db)
    d = _NMR_DESIGNS.get(key)
    if d is not None:
        return d
    N, nb = n_fft, n_fft // 2 + 1
    k = np.arange(nb, dtype=np.float64)
    f = k[1:] * (fs / N) / 1000.0
    w = np.zeros(nb)
    w[1:] = 10.0 ** ((-2.184 * f ** -0.8 + 6.5 * np.exp(-0.6 * (f - 3.3) ** 2) - 0.001 * f ** 3.6) / 10.0)
    w *= 10.0 ** (level_db / 10.0) / (N / 4.0) ** 2
    zl, zu = 7.0 * math.asinh(80.0 / 650.0), 7.0 * math.asinh(min(18000.0, 0.45 * fs) / 650.0)
    Nc = int(math.ceil((zu - zl) / NMR_DZ))
    lo = zl + NMR_DZ * np.arange(Nc)
    hi = np.minimum(lo + NMR_DZ, zu)
    fl, fu, fc = 650.0 * np.sinh(lo / 7.0), 650.0 * np.sinh(hi / 7.0), 650.0 * np.sinh(0.5 * (lo + hi) / 7.0)
    width = fs / N
    # bin k occupies [(k - 1/2), (k + 1/2)] width: a band's first and last bin and the share of each that lies inside the band
    k_lo = np.floor(fl / width + 0.5).astype(np.int64)
    k_hi = np.minimum(np.ceil(fu / width - 0.5).astype(np.int64), nb - 1)
    k_hi = np.maximum(k_hi, k_lo)
    share = lambda kk, i: max(min((kk + 0.5) * width, fu[i]) - max((kk - 0.5) * width, fl[i]), 0.0) / width      # noqa: E731
    u_lo = np.array([share(k_lo[i], i) for i in range(Nc)])
    u_hi = np.array([share(k_hi[i], i) for i in range(Nc)])
    table = np.zeros((Nc, 8))
    table[:, 0], table[:, 1] = u_lo, u_hi
    table[:, 2] = 10.0 ** (0.1456 * (fc / 1000.0) ** -0.8)
    table[:, 3] = -24.0 - 230.0 / fc
    rd = 10.0 ** (-2.7 * NMR_DZ)
    table[:, 4] = np.concatenate(([0.0], np.cumsum(rd ** np.arange(1, Nc))))
    # Bs: the spreading of Eb = 1 in every band, in the definition's direct form
    i_, l_ = np.arange(Nc)[:, None], np.arange(Nc)[None, :]
    S = np.where(i_ >= l_, 10.0 ** (table[:, 3][None, :] * (i_ - l_) * NMR_DZ / 10.0), 10.0 ** (-2.7 * (l_ - i_) * NMR_DZ))
    S = S / S.sum(axis=0, keepdims=True)
    table[:, 5] = 1.0 / ((S ** 0.4).sum(axis=1) ** 2.5)
    table[:, 6] = np.exp(-((N // 2) / fs) / (0.008 + (100.0 / fc) * 0.022))
    m_db = np.where(np.arange(Nc) <= 12.0 / NMR_DZ, 3.0, 0.25 * np.arange(Nc) * NMR_DZ)
    table[:, 7] = 10.0 ** (-m_db / 10.0)
    d = {"n_fft": N, "level_db": level_db, "fc": fc, "weights": np.ascontiguousarray(w),
         "bins": np.ascontiguousarray(np.stack([k_lo, k_hi], axis=1).astype(np.int32)), "table": np.ascontiguousarray(table), "mask_db": m_db}
    _NMR_DESIGNS[key] = d
    return d


def nmr_metrics(tgt_list, est_list, tgt_index, fs, n_fft=None, level_db=NMR_LEVEL_DB, split_bands=None, return_bands=False,
                return_mask=False, device=None, deferred=False):
    """The noise-to-mask ratio of estimate e against target tgt_index[e] (ssr_nmr): waveforms at rate fs (float32 or
    float64, each estimate as long as its target; a list holding both dtypes is widened to float64) -> (rows [n_est, 6] float64: nmr,
    nmr_seg, rdf, nmr_hf, nmr_lf, frames; bands [n_est, Nc]: mean_t R per band, or None without return_bands; mask [the frames of all
    targets, Nc]: the masking threshold M of every target, frame after frame in target order, or None without return_mask).  n_fft:
    None = nmr_default_nfft(fs), or 256, 512, 1024 or 2048 (hop n_fft / 2); split_bands: None, or per estimate the first band of its
    upper part in [0, Nc] (-1: no split).  The workspace holds 8 Nc bytes per frame of every target and 8 (Nc + 2) bytes per chunk of
    32 frames of every pair.  Device views of one buffer are read where they lie.  deferred: a function that returns the tuple."""
    d = nmr_design(fs, n_fft, level_db)
    n_fft, J = d["n_fft"], d["fc"].shape[0]
    if not isinstance(return_bands, (bool, np.bool_)) or not isinstance(return_mask, (bool, np.bool_)):
        raise ValueError("return_bands and return_mask must be True or False")
    tgts, ests, idx = _signal_pair_index(tgt_list, est_list, tgt_index)
    n_t, n_e = len(tgts), len(ests)
    sp = _split_array(split_bands, n_e, lambda s: s.min() >= -1 and s.max() <= J, "split_bands must hold -1 or a band in [0, n_bands] per estimate")
    lib, dev = _gpu_call(device)
    with torch.cuda.device(dev):
        rows = torch.empty((n_e, NMR_COLUMNS), dtype=torch.float64, device=dev)
        bands = torch.empty((n_e, J), dtype=torch.float64, device=dev) if return_bands else None
        mask = None
        if n_e:
            tgt_side, est_side, tl = _signal_pair_place(tgts, ests, idx, dev)
            lens = tl.astype(np.int32)
            frames = int(np.where(lens >= n_fft, 1 + (lens - n_fft) // (n_fft // 2), 0).sum())
            mask = torch.empty((frames, J), dtype=torch.float64, device=dev) if return_mask else None
            ws_bytes = int(lib.ssr_nmr_workspace_bytes(lens.ctypes.data_as(C.c_void_p), n_t, idx.ctypes.data_as(C.c_void_p), n_e, n_fft, J))
            ws = _workspace(ws_bytes, dev)
            lens_h, idx_h, sp_h, bins_h = _host_i32(lens, dev), _host_i32(idx, dev), _host_i32(sp, dev), _host_i32(d["bins"], dev)
            # the weights stay on the device for the life of the process, one table (at most 8 KB) per (rate, n_fft, level, device); the
            # band table is read by the library out of page-locked memory, like the int32 arrays: no copy waits for the stream
            key = (float(fs), n_fft, d["level_db"], torch.cuda.current_device())
            w_dev = _NMR_WEIGHTS.get(key)
            if w_dev is None:
                w_dev = _NMR_WEIGHTS[key] = _h2d(d["weights"], dev)
            tab_h = _DescRing.get(torch.cuda.current_device()).stage(d["table"], dev)
            _lib.check(lib.ssr_nmr(*_args(tgt_side), _vp(lens_h), n_t, *_args(est_side), _vp(idx_h), n_e, n_fft, J, _vp(w_dev), _vp(bins_h),
                                   _vp(tab_h), _vp(sp_h), _vp(rows), _vp(bands), _vp(mask), _vp(ws), ws_bytes, _stream()))
        elif return_mask:
            mask = torch.empty((0, J), dtype=torch.float64, device=dev)
        return _collected([_take(rows), _take(bands) if return_bands else (lambda: None), _take(mask) if return_mask else (lambda: None)], deferred)


# ---- delay estimation and compensation: a stage in front of the metrics ----------------------------------------------------
ALIGN_MAX_LAG = _lib.ALIGN_MAX_LAG       # SSR_ALIGN_MAX_LAG
ALIGN_LAG = 1024                         # the default search range in samples, either way
ALIGN_COLUMNS = _lib.ALIGN_COLUMNS       # SSR_ALIGN_COLUMNS: delay, frac, corr, edge


def check_align_lag(max_lag):
    """max_lag as an int, or ValueError: an integer in [1, 4096] (the C ABI's own check)."""
    if isinstance(max_lag, bool) or not isinstance(max_lag, (int, np.integer)) or not 1 <= int(max_lag) <= ALIGN_MAX_LAG:
        raise ValueError("max_lag must be an integer in [1, %d]" % ALIGN_MAX_LAG)
    return int(max_lag)


def check_align_subsample(subsample):
    """subsample as a bool, or ValueError."""
    if not isinstance(subsample, (bool, np.bool_)):
        raise ValueError("subsample must be True or False")
    return bool(subsample)


def align(tgt_list, est_list, tgt_index, max_lag=ALIGN_LAG, subsample=False, return_corr=False, device=None, deferred=False, shift=True):
    """The delay of estimate e against target tgt_index[e] and the estimate with that delay taken out (ssr_align):
    waveforms (float32 or float64; an estimate need NOT be as long as its target; targets of both dtypes are widened to float64,
    estimates of both dtypes go through one call per dtype) -> (rows [n_est, 4] float64: delay d* in samples (positive: the estimate
    is late), the parabola's sub-sample estimate frac in [-0.5, 0.5], the normalised correlation at d*, edge = 1 where |d*| = max_lag;
    shifted: a list of n_est DEVICE tensors in each estimate's dtype and length, z[t] = y[t + d*] with zero fill - with subsample and
    frac != 0 through a 33-tap windowed sinc at d* + frac -, views of one buffer per dtype that stay in HBM (None with shift=False);
    c [n_est, 2 max_lag + 1], lag -max_lag first, or None without return_corr).  A silent or empty signal on either side, and a
    correlation that is nowhere positive: delay 0, frac 0, edge 0, corr NaN, the estimate unchanged.  The delay found reaches the
    shift through device memory: nothing waits on the host.  Device views of one buffer are read where they lie.  deferred: rows
    and c are functions that return the arrays."""
    L, subsample = check_align_lag(max_lag), check_align_subsample(subsample)
    if not isinstance(return_corr, (bool, np.bool_)) or not isinstance(shift, (bool, np.bool_)):
        raise ValueError("return_corr and shift must be True or False")
    tgts, ests, idx = _signal_pair_index(tgt_list, est_list, tgt_index)
    n_e = len(ests)
    lib, dev = _gpu_call(device)
    groups = {}
    for e, w in enumerate(ests):
        groups.setdefault(bool(_is_f64(w)), []).append(e)
    shifted = [None] * n_e if shift else None
    got = []
    with torch.cuda.device(dev):
        for f64, members in groups.items():
            used = sorted({int(idx[e]) for e in members})
            where = {t: j for j, t in enumerate(used)}
            sub_idx = np.array([where[int(idx[e])] for e in members], dtype=np.int32)
            tgt_side, est_side, tl, el = _placed_where_they_lie([tgts[t] for t in used], [ests[e] for e in members], sub_idx, dev)
            n_t, n_g = len(used), len(members)
            rows = torch.empty((n_g, ALIGN_COLUMNS), dtype=torch.float64, device=dev)
            c = torch.empty((n_g, 2 * L + 1), dtype=torch.float64, device=dev) if return_corr else None
            out, out_off = None, None
            if shift:
                out = torch.empty(int(el.sum()), dtype=torch.float64 if f64 else torch.float32, device=dev)
                out_off = _h2d(_offsets(el), dev)
                edges = np.concatenate(([0], np.cumsum(el))).astype(np.int64)
                for j, e in enumerate(members):
                    shifted[e] = out[edges[j]:edges[j + 1]]
            lens, elens = tl.astype(np.int32), el.astype(np.int32)
            as_p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
            ws_bytes = int(lib.ssr_align_workspace_bytes(as_p(lens), n_t, as_p(elens), as_p(sub_idx), n_g, L))
            ws = _workspace(ws_bytes, dev)
            lens_h, elens_h, idx_h = _host_i32(lens, dev), _host_i32(elens, dev), _host_i32(sub_idx, dev)
            _lib.check(lib.ssr_align(*_args(tgt_side), _vp(lens_h), n_t, *_args(est_side), _vp(elens_h), _vp(idx_h), n_g, L, int(subsample),
                                     _vp(rows), _vp(out) if out is not None and out.numel() else None, _vp(out_off), _vp(c), _vp(ws),
                                     ws_bytes, _stream()))
            got.append((members, _take(rows), _take(c) if return_corr else None))

    def collect_rows():
        full = np.empty((n_e, ALIGN_COLUMNS))
        for members, r, _ in got:
            full[members] = r()
        return full

    def collect_corr():
        full = np.empty((n_e, 2 * L + 1))
        for members, _, c in got:
            full[members] = c()
        return full
    if deferred:
        return collect_rows, shifted, (collect_corr if return_corr else None)
    return collect_rows(), shifted, (collect_corr() if return_corr else None)


# ---- distribution: Fréchet and kernel distance of embedding sets ---------------------------------------------------------
DISTRIBUTION_MAX_DIM = 1024              # SSR_DISTRIBUTION_MAX_DIM
DISTRIBUTION_MAX_GAMMA = 8               # SSR_DISTRIBUTION_MAX_GAMMA
DISTRIBUTION_MAX_PAIR_ROWS = 2048        # SSR_DISTRIBUTION_MAX_PAIR_ROWS
DISTRIBUTION_MAX_SWEEPS = 60             # the default bound of the Jacobi's sweep loop
FRECHET_COLUMNS = 8                      # SSR_FRECHET_COLS: fd, |dmu|^2, tr Sigma_r, tr Sigma_e, tr_sqrt, sweeps_ref, sweeps_est, rank_ref
KERNEL_DISTANCE_COLUMNS = 4              # SSR_KERNEL_DISTANCE_COLS: kd, mmd2, mean k(r, r), mean k(e, e)


def check_distribution_max_sweeps(max_sweeps):
    """max_sweeps as an int, or ValueError: a whole number in [1, 200] (the C ABI's own check)."""
    if isinstance(max_sweeps, (bool, np.bool_)) or not isinstance(max_sweeps, (int, np.integer)) or not 1 <= max_sweeps <= 200:
        raise ValueError("max_sweeps must be a whole number in [1, 200]")
    return int(max_sweeps)


def check_distribution_gammas(gammas):
    """The kernel bandwidths as a float64 array, or ValueError: 1 to 8 finite values > 0."""
    try:
        if isinstance(gammas, (str, bytes)):
            raise TypeError
        g = np.ascontiguousarray(gammas, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("gamma must hold 1 to 8 finite values > 0")
    if not 1 <= g.shape[0] <= DISTRIBUTION_MAX_GAMMA or not np.all(np.isfinite(g) & (g > 0.0)):
        raise ValueError("gamma must hold 1 to 8 finite values > 0")
    return g


def check_distribution_scale(scale):
    if isinstance(scale, (bool, np.bool_)) or not isinstance(scale, (int, float, np.integer, np.floating)) or not math.isfinite(scale):
        raise ValueError("scale must be a finite number")
    return float(scale)


def _embedding_set(s, what):
    """A set of embeddings as a 2-D float32 / float64 tensor (wherever it lives), or ValueError."""
    t = s if isinstance(s, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(s))
    if t.dim() != 2 or t.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s must be a 2-D float32 or float64 array [rows, D]" % what)
    if not 1 <= t.shape[1] <= DISTRIBUTION_MAX_DIM:
        raise ValueError("%s must have 1 <= D <= %d columns" % (what, DISTRIBUTION_MAX_DIM))
    return t


def _distribution_sets(ref, ests):
    """The reference and the estimate sets checked -> (tensors, D); nothing touches a device."""
    if isinstance(ests, (torch.Tensor, np.ndarray)):
        raise ValueError("ests must be a list of sets")
    ts = [_embedding_set(ref, "ref")] + [_embedding_set(e, "every estimate set") for e in ests]
    if len(ts) < 2:
        raise ValueError("at least one estimate set")
    if any(t.shape[1] != ts[0].shape[1] for t in ts):
        raise ValueError("every set must have the reference's D")
    return ts, int(ts[0].shape[1])


def _distribution_pack(ts, dev):
    """The sets back to back in one device buffer of their widest dtype -> (data, is-float64, element offsets int64, rows int64)."""
    dt = torch.float64 if any(t.dtype == torch.float64 for t in ts) else torch.float32
    data = torch.cat([t.to(device=dev, dtype=dt) for t in ts], dim=0).contiguous()
    rows = np.array([t.shape[0] for t in ts], np.int64)
    return data, int(dt == torch.float64), (np.cumsum(rows) - rows) * int(ts[0].shape[1]), rows


def frechet_stats(ref, ests, max_sweeps=DISTRIBUTION_MAX_SWEEPS, return_moments=False, device=None):
    """ssr_frechet on the reference set ref [n, D] and the list of estimate sets ests (each [m_k, D]); torch tensors or
    NumPy arrays, float32 or float64 (mixed: widened to float64), resident or host -> out [K, 8] float64 = fd, |mu_r - mu_e|^2,
    tr Sigma_r, tr Sigma_e, tr sqrt(Sigma_r Sigma_e), sweeps_ref, sweeps_est, rank_ref; with return_moments (out, moments [1 + K, D + D D]:
    mean and row-major covariance of every set)."""
    ts, D = _distribution_sets(ref, ests)
    max_sweeps = check_distribution_max_sweeps(max_sweeps)
    require_gpu()
    lib = _lib.load()
    dev = torch.device(device) if device is not None else default_device()
    K = len(ts) - 1
    with torch.cuda.device(dev):
        data, f64, off, rows = _distribution_pack(ts, dev)
        out = torch.empty((K, FRECHET_COLUMNS), dtype=torch.float64, device=dev)
        mom = torch.empty((K + 1, D + D * D), dtype=torch.float64, device=dev) if return_moments else None
        ws_bytes = int(lib.ssr_frechet_workspace_bytes(rows.ctypes.data_as(C.c_void_p), K, D))
        if ws_bytes == 0:
            raise SsrHipError("sets too large for one ssr_frechet call")
        ws = _workspace(ws_bytes, dev)
        _lib.check(lib.ssr_frechet(_vp(data), f64, off.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), K, D, D, max_sweeps,
                                   _vp(out), _vp(mom), _vp(ws), ws_bytes, _stream()))
        res = out.cpu().numpy()
        return (res, mom.cpu().numpy()) if return_moments else res


def kernel_sums(ref, ests, gammas, scale=1000.0, device=None):
    """ssr_kernel_distance: the unbiased MMD^2 with the Gaussian kernels exp(-gamma |x - y|^2) of the reference set and
    every estimate set (inputs as frechet_stats takes them; gammas: 1 to 8 values) -> [K, n_gamma, 4] float64 = kd = scale mmd2, mmd2,
    mean k(r, r), mean k(e, e)."""
    ts, D = _distribution_sets(ref, ests)
    g = check_distribution_gammas(gammas)
    scale = check_distribution_scale(scale)
    require_gpu()
    lib = _lib.load()
    dev = torch.device(device) if device is not None else default_device()
    K = len(ts) - 1
    with torch.cuda.device(dev):
        data, f64, off, rows = _distribution_pack(ts, dev)
        out = torch.empty((K, len(g), KERNEL_DISTANCE_COLUMNS), dtype=torch.float64, device=dev)
        ws_bytes = int(lib.ssr_kernel_distance_workspace_bytes(rows.ctypes.data_as(C.c_void_p), K, D, len(g)))
        if ws_bytes == 0:
            raise SsrHipError("sets too large for one ssr_kernel_distance call")
        ws = _workspace(ws_bytes, dev)
        _lib.check(lib.ssr_kernel_distance(_vp(data), f64, off.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), K, D, D,
                                           g.ctypes.data_as(C.c_void_p), len(g), scale, _vp(out), _vp(ws), ws_bytes, _stream()))
        return out.cpu().numpy()


def pairwise_distances(x, index=None, device=None, as_tensor=False):
    """ssr_pairwise_distances: |x_i - x_j|, i < j, of the rows index (default: all; at most 2048) of the set x [rows, D] -> float64
    [n (n - 1) / 2] in row-major order of the upper triangle, as an ndarray or (as_tensor) a device tensor."""
    t = _embedding_set(x, "x")
    idx = np.arange(t.shape[0], dtype=np.int64) if index is None else np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
    n = len(idx)
    if n > DISTRIBUTION_MAX_PAIR_ROWS:
        raise ValueError("at most %d rows" % DISTRIBUTION_MAX_PAIR_ROWS)
    if n and (idx.min() < 0 or idx.max() >= t.shape[0]):
        raise ValueError("index out of range")
    require_gpu()
    lib = _lib.load()
    dev = torch.device(device) if device is not None else default_device()
    with torch.cuda.device(dev):
        data = t.to(dev).contiguous()
        out = torch.empty(n * (n - 1) // 2, dtype=torch.float64, device=dev)
        ws = _workspace(_lib.DISTRIBUTION_PAIRWISE_WORKSPACE, dev)
        _lib.check(lib.ssr_pairwise_distances(_vp(data), int(t.dtype == torch.float64), 0, t.shape[0], t.shape[1], t.shape[1],
                                              idx.ctypes.data_as(C.c_void_p), n, _vp(out), _vp(ws), _lib.DISTRIBUTION_PAIRWISE_WORKSPACE, _stream()))
        return out if as_tensor else out.cpu().numpy()


# ---- pitch: YIN F0 tracks, F0 RMSE, F0 correlation, GPE, VDE and FFE ------------------------------------------------------------
PITCH_FS = 16000                 # the rate every signal is tracked at
PITCH_HOP = 160


def check_pitch_range(fmin, fmax):
    """(fmin, fmax) as floats, or ValueError: 40 <= fmin < fmax <= 1000 and at least three lags in [floor(16000 / fmax),
    ceil(16000 / fmin)] (the C ABI's own check)."""
    fmin, fmax = float(fmin), float(fmax)
    if not 40.0 <= fmin < fmax <= 1000.0:
        raise ValueError("fmin / fmax must satisfy 40 <= fmin < fmax <= 1000")
    if math.ceil(PITCH_FS / fmin) - math.floor(PITCH_FS / fmax) < 2:
        raise ValueError("fmin / fmax leave fewer than three lags")
    return fmin, fmax


def pitch_frames(n16):
    """Frames of a 16 kHz signal of n16 samples (10 ms hop, frame t centred on sample 160 t)."""
    return int(n16) // PITCH_HOP + 1 if int(n16) > 0 else 0


def resample_to_pitch_rate(wavs, fs, device=None):
    """The 16 kHz float64 signals the tracker analyses: [float32 / float64 waveforms at fs] -> Ragged float64, in one
    ssr_resample_poly_f64 launch with SciPy's default Kaiser design (bit-identical to scipy.signal.resample_poly(x64, 16000 // g,
    fs // g)); at 16 kHz the signals, widened."""
    if not 8000 <= int(fs) <= 48000:
        raise ValueError("the pitch metrics need 8000 <= fs <= 48000")
    dev = torch.device(device) if device is not None else default_device()
    with torch.cuda.device(dev):
        return _resample_f64(wavs, ResamplePlan.get(PITCH_FS, int(fs), dev), dev)


def f0_track(wavs, fs, fmin=50.0, fmax=500.0, device=None):
    """YIN F0 tracks (ssr_f0_track) of waveforms at `fs` (float32 or float64; resampled to 16 kHz in one launch) ->
    one (f0 [T], voiced [T] bool, aperiodicity [T], energy [T]) tuple of float64 / bool ndarrays per signal, 10 ms frames."""
    require_gpu()
    fmin, fmax = check_pitch_range(fmin, fmax)
    dev = torch.device(device) if device is not None else default_device()
    n = len(wavs)
    if n == 0:
        return []
    lib = _lib.load()
    with torch.cuda.device(dev):
        r = resample_to_pitch_rate(list(wavs), fs, dev)
        lens = r.lens_host.astype(np.int32)
        T = np.array([pitch_frames(m) for m in lens], np.int64)
        foff = _offsets(T)
        tot = max(int(T.sum()), 1)
        f0, ap, en = (torch.empty(tot, dtype=torch.float64, device=dev) for _ in range(3))
        vo = torch.empty(tot, dtype=torch.uint8, device=dev)
        ws_bytes = int(lib.ssr_f0_track_workspace_bytes(lens.ctypes.data_as(C.c_void_p), n, fmin, fmax))
        ws = _workspace(ws_bytes, dev)
        lens_h = _host_i32(lens, dev)
        foff_d = _h2d(foff, dev)
        _lib.check(lib.ssr_f0_track(_vp(r.data), _vp(r.off), _vp(lens_h), n, fmin, fmax, _vp(f0), _vp(ap), _vp(en), _vp(vo), _vp(foff_d),
                                    _vp(ws), ws_bytes, _stream()))
        f0, ap, en, vo = (t.cpu().numpy() for t in (f0, ap, en, vo))
    return [(f0[a:a + t], vo[a:a + t].astype(bool), ap[a:a + t], en[a:a + t]) for a, t in zip(foff, T)]


def pitch_metrics(tgt_list, est_list, tgt_index, fs, which=31, fmin=50.0, fmax=500.0, device=None, deferred=False):
    """F0 RMSE / F0 correlation / GPE / VDE / FFE of estimate e against target tgt_index[e] (ssr_f0_metrics): waveforms
    at `fs` (float32 or float64, each estimate as long as its target) -> [n_est, n_out] float64, columns in bit order of `which`
    (1 f0_rmse, 2 f0_corr, 4 gpe, 8 vde, 16 ffe).  Targets and estimates are resampled to 16 kHz in one launch; every target is
    tracked once for all its estimates.  deferred: a Pending."""
    which = int(which)
    if not 1 <= which <= 31:
        raise ValueError("which must be a non-empty combination of 1 (f0_rmse), 2 (f0_corr), 4 (gpe), 8 (vde) and 16 (ffe)")
    fmin, fmax = check_pitch_range(fmin, fmax)
    if not 8000 <= int(fs) <= 48000:
        raise ValueError("the pitch metrics need 8000 <= fs <= 48000")
    lib = _lib.load()

    def place(tgts, ests, idx, dev):
        # the lengths are compared BEFORE resampling (two lengths at fs can round to one at 16 kHz)
        n_in = np.array([int(a.shape[0]) for a in tgts + ests], np.int64)
        if not np.array_equal(n_in[len(tgts):], n_in[:len(tgts)][idx]):
            raise ValueError("every estimate must be as long as its target (truncate to the common length first)")
        return _placed_resampled(resample_to_pitch_rate(tgts + ests, fs, dev), len(tgts))
    return _pair_index_metrics(tgt_list, est_list, tgt_index, bin(which).count("1"), place,
                               lambda *a: lib.ssr_f0_metrics_workspace_bytes(*a, fmin, fmax, which), lib.ssr_f0_metrics,
                               (fmin, fmax, which), device, deferred)


BOOTSTRAP_SCHEMES = {"utterance": _lib.BOOTSTRAP_UTTERANCE, "speaker": _lib.BOOTSTRAP_SPEAKER}


def bootstrap_geometry():
    """(index_tile, max_boot) of ssr_bootstrap_geometry: the file draws a workgroup generates at a time and the largest n_boot.
    Host only."""
    tile, cap = C.c_int(), C.c_int()
    _lib.check(_lib.load().ssr_bootstrap_geometry(C.byref(tile), C.byref(cap)))
    return tile.value, cap.value


def bootstrap_means(table, spk_off, n_boot, seed=0, scheme="utterance", device=None):
    """Bootstrap replicates of the mean-of-speaker-means aggregate (ssr_bootstrap_means): table [N, K] float64 (ndarray
    or tensor; rows grouped by speaker, speaker s at spk_off[s] .. spk_off[s + 1] - 1) -> device tensor [n_boot, K] float64.  The
    same drawn files serve every column; a column with a non-finite entry is NaN in every replicate."""
    require_gpu()
    if scheme not in BOOTSTRAP_SCHEMES:
        raise ValueError("resample must be 'utterance' or 'speaker'")
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in [0, 2^64)")
    dev = torch.device(device) if device is not None else default_device()
    spk_off = np.ascontiguousarray(spk_off, dtype=np.int32)
    with torch.cuda.device(dev):
        t = table if isinstance(table, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(table, dtype=np.float64))
        t = t.to(device=dev, dtype=torch.float64).contiguous()
        if t.dim() != 2:
            raise ValueError("table must be [files, columns]")
        N, K = int(t.shape[0]), int(t.shape[1])
        reps = torch.empty((max(int(n_boot), 0), K), dtype=torch.float64, device=dev)
        _lib.check(_lib.load().ssr_bootstrap_means(_vp(t), N, K, spk_off.ctypes.data_as(C.c_void_p), len(spk_off) - 1, int(n_boot), seed,
                                                   BOOTSTRAP_SCHEMES[scheme], _vp(reps), _stream()))
    return reps


def bootstrap_summary(reps, q):
    """Per column of the device tensor reps [B, K] float64 (ssr_bootstrap_summary): (mean [K], standard error [K] (ddof 1),
    quantiles [len(q), K] by NumPy's linear rule, n_le0 [K], n_ge0 [K]) as ndarrays; a column holding a non-finite replicate: NaN
    and -1."""
    require_gpu()
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    if not (isinstance(reps, torch.Tensor) and reps.is_cuda and reps.dtype == torch.float64 and reps.dim() == 2):
        raise ValueError("reps must be a [B, K] float64 device tensor")
    reps = reps.contiguous()
    B, K = int(reps.shape[0]), int(reps.shape[1])
    with torch.cuda.device(reps.device):
        out = torch.empty((K, 2 + len(q)), dtype=torch.float64, device=reps.device)
        counts = torch.empty((K, 2), dtype=torch.int32, device=reps.device)
        _lib.check(_lib.load().ssr_bootstrap_summary(_vp(reps), B, K, q.ctypes.data_as(C.c_void_p), len(q), _vp(out), _vp(counts),
                                                     _stream()))
        out, counts = out.cpu().numpy(), counts.cpu().numpy()
    return out[:, 0].copy(), out[:, 1].copy(), np.ascontiguousarray(out[:, 2:].T), counts[:, 0].copy(), counts[:, 1].copy()


def stft(plan, wavs, kind="mag", torch_style_pad=False):
    """STFT of a list of waveforms.  kind "mag": list of [T, F] tensors; "complex": (re list, im list).
    torch_style_pad: refuse signals not longer than n_fft//2 the way torch's reflect padding does (torchlibrosa);
    otherwise short signals are reflect-padded repeatedly, as numpy.pad / librosa do."""
    with torch.cuda.device(plan.device):
        r = wavs if isinstance(wavs, Ragged) else Ragged.from_list(wavs, plan.device)
        if r.n == 0:
            return ([], []) if kind == "complex" else []
        if torch_style_pad:
            _check_reflect(plan, r.lens_host)
        _check_nonempty(r.lens_host)
        rows = _Rows(plan, r.lens_host, r.device)
        a = torch.empty((rows.total, plan.n_bins), dtype=torch.float32, device=r.device)
        b = torch.empty_like(a) if kind == "complex" else None
        _lib.check(plan.lib.ssr_stft(plan.handle, _vp(r.data), _vp(r.off), _vp(r.len), _vp(rows.off), r.n, r.max_len,
                                     _lib.STFT_COMPLEX if kind == "complex" else _lib.STFT_MAG, _vp(a), _vp(b), _stream()))
        cut = lambda m: [m[rows.off_host[i]:rows.off_host[i] + rows.T[i]] for i in range(r.n)]
        return (cut(a), cut(b)) if kind == "complex" else cut(a)


def magphase(re, im, eps):
    """(mag, cos, sin) of ssr_eval/dsp.py:76-81 for float32 device tensors of any shape."""
    re, im = re.contiguous(), im.contiguous()
    mag, cos, sin = torch.empty_like(re), torch.empty_like(re), torch.empty_like(re)
    with torch.cuda.device(re.device):
        _lib.check(_lib.load().ssr_magphase(_vp(re), _vp(im), re.numel(), float(eps), _vp(mag), _vp(cos), _vp(sin), _stream()))
    return mag, cos, sin


def _dev_f32(x, dev=None):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    dev = dev if dev is not None else (t.device if t.is_cuda else default_device())
    return t.to(device=dev, dtype=torch.float32).contiguous()


def elementwise(op, x):
    """op "to_log": log10(x + 1e-12); "from_log": 10 ** min(x, 5) (ssr_eval/utils.py:43-50).  float32 device tensor."""
    require_gpu()
    t = _dev_f32(x)
    out = torch.empty_like(t)
    fn = {"to_log": _lib.load().ssr_to_log, "from_log": _lib.load().ssr_from_log}[op]
    with torch.cuda.device(t.device):
        _lib.check(fn(_vp(t), t.numel(), _vp(out), _stream()))
    return out


def energy_sums(a, b, n_items):
    """[n_items, 3] float64 device tensor {sum a^2, sum b^2, sum a*b} over n_items equal contiguous slices."""
    require_gpu()
    ta = _dev_f32(a)
    tb = _dev_f32(b, ta.device)
    if ta.shape != tb.shape or n_items <= 0 or ta.numel() % n_items:
        raise ValueError("energy_sums needs two tensors of one shape that split evenly into n_items slices")
    out = torch.empty((n_items, 3), dtype=torch.float64, device=ta.device)
    with torch.cuda.device(ta.device):
        _lib.check(_lib.load().ssr_energy_sums(_vp(ta), _vp(tb), n_items, ta.numel() // n_items, _vp(out), _stream()))
    return out


def scale_items(x, mul, div):
    """(x[i] * mul[i]) / div[i] per leading-dimension slice, float32 with two roundings (energy_unify)."""
    require_gpu()
    t = _dev_f32(x)
    m, d = _dev_f32(mul, t.device).reshape(-1), _dev_f32(div, t.device).reshape(-1)
    n_items = m.numel()
    if d.numel() != n_items or n_items == 0 or t.numel() % n_items:
        raise ValueError("one multiplier and one divisor per slice")
    out = torch.empty_like(t)
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().ssr_scale_items(_vp(t), _vp(m), _vp(d), n_items, t.numel() // n_items, _vp(out), _stream()))
    return out


def sispec_multichannel(est, target, log_domain):
    """SISpec (or its to_log variant) of [B, C, T, F] tensors with C > 1 -> 0-dim float64 device tensor (the batch mean)."""
    require_gpu()
    e = _dev_f32(est)
    t = _dev_f32(target, e.device)
    Bn, Cn = int(e.shape[0]), int(e.shape[1])
    per = e[0, 0].numel()
    out = torch.empty(Bn + 1, dtype=torch.float64, device=e.device)
    ws = torch.empty(Bn * Cn * 3, dtype=torch.float64, device=e.device)
    with torch.cuda.device(e.device):
        _lib.check(_lib.load().ssr_sispec_multichannel(_vp(e), _vp(t), Bn, Cn, per, 1 if log_domain else 0, _vp(out), _vp(ws),
                                                       ws.numel() * 8, _stream()))
    return out[Bn]


def spectrogram_metrics(est_sps, tgt_sps, mask=M_ALL):
    """Metrics on lists of [T_i, F] float32 magnitude spectrograms -> [n, 4] float64 device tensor."""
    require_gpu()
    lib = _lib.load()
    dev = est_sps[0].device if isinstance(est_sps[0], torch.Tensor) and est_sps[0].is_cuda else default_device()
    with torch.cuda.device(dev):
        to_dev = lambda s: (s if isinstance(s, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(s))).to(
            device=dev, dtype=torch.float32)
        es, ts = [to_dev(s) for s in est_sps], [to_dev(s) for s in tgt_sps]
        F = es[0].shape[1]
        for e, t in zip(es, ts):
            if e.shape != t.shape or e.dim() != 2 or e.shape[1] != F:
                raise ValueError("spectrogram shape mismatch")
        T = np.array([e.shape[0] for e in es], dtype=np.int64)
        if (mask & M_SSIM) and (T.min() < 7 or F < 7):
            raise ValueError("win_size exceeds image extent")
        x = torch.cat([e.reshape(-1) for e in es])
        y = torch.cat([t.reshape(-1) for t in ts])
        off = _h2d(_offsets(T), dev)
        rows = _h2d(T.astype(np.int32), dev)
        n, max_T = len(es), int(T.max())
        ws_bytes = int(lib.ssr_spectrogram_metrics_workspace_bytes(n, max_T, F))
        ws = _workspace(ws_bytes, dev)
        out = torch.empty((n, 4), dtype=torch.float64, device=dev)
        _lib.check(lib.ssr_spectrogram_metrics(_vp(x), _vp(y), _vp(off), _vp(rows), n, max_T, F, mask, _vp(out), _vp(ws),
                                               ws_bytes, _stream()))
        return out


class LowpassBatch:
    """A ragged batch + cached descriptors / workspace / output for repeated ssr_fft_lowpass calls (K6): one cut bin per
    item.  `run()` enqueues the launch sequence on the current stream and returns the flat output buffer (same layout as
    the input batch); `out_ragged()` views it as a Ragged batch for the metric stage."""

    def __init__(self, plan, ragged, cut_bins, out=None):
        _check_reflect(plan, ragged.lens_host)
        if ragged.data.dtype != torch.float32:
            raise ValueError("the STFT-domain low-pass takes float32 signals (torchlibrosa's convolution does too)")
        self.plan, self.r = plan, ragged
        self.rows = _Rows(plan, ragged.lens_host, ragged.device)
        self.set_cuts(cut_bins)
        self.ws_bytes = int(plan.lib.ssr_ola_workspace_bytes(plan.handle, self.rows.total))
        self.ws = _workspace(self.ws_bytes, ragged.device)
        # out: a caller-owned float32 buffer of the batch's size (e.g. one key's slice of a multi-key estimate buffer)
        if out is not None and (out.dtype != torch.float32 or out.numel() != ragged.data.numel() or not out.is_contiguous()):
            raise ValueError("out must be a contiguous float32 buffer of the batch's size")
        self.out = out if out is not None else torch.empty_like(ragged.data)

    def set_cuts(self, cut_bins):
        """One cut bin per item (a scalar: the same for every item).  A batch with ONE cut runs through ssr_fft_lowpass_multi (row
        tiles across item boundaries), per-item cuts through ssr_fft_lowpass."""
        cuts = np.asarray(cut_bins, dtype=np.int32).reshape(-1)
        if cuts.size == 1 and self.r.n != 1:
            cuts = np.repeat(cuts, self.r.n)
        if cuts.size != self.r.n:
            raise ValueError("one cut bin per item")
        self.uniform = int(cuts[0]) if cuts.size and bool((cuts == cuts[0]).all()) else None
        self.cut = _h2d(cuts, self.r.device)

    def run(self):
        p, r = self.plan, self.r
        if not r.n:
            return self.out
        if self.uniform is not None:
            # one cut for the whole batch: the launch's row tiles run across item boundaries (ssr_fft_lowpass_multi with one key)
            cuts = (C.c_int32 * 1)(self.uniform)
            _lib.check(p.lib.ssr_fft_lowpass_multi(p.handle, _vp(r.data), _vp(r.off), _vp(r.len), cuts, 1, _vp(self.rows.off), r.n,
                                                   r.max_len, self.rows.total, _vp(self.out), 0, _vp(self.ws), self.ws_bytes, _stream()))
        else:
            _lib.check(p.lib.ssr_fft_lowpass(p.handle, _vp(r.data), _vp(r.off), _vp(r.len), _vp(self.cut), _vp(self.rows.off),
                                             r.n, r.max_len, self.rows.total, _vp(self.out), _vp(self.ws), self.ws_bytes,
                                             _stream()))
        return self.out

    def out_ragged(self):
        return Ragged(self.out, self.r.off, self.r.len, self.r.lens_host)


class MultiLowpassBatch:
    """One ragged batch, K cut bins applied to every item (SSR_Eval_Helper.lowpass_stft_hard's loop over setting_fft,
    ssr_eval/eval.py:401-410): ssr_fft_lowpass_multi.  `run()` returns the [K, batch samples] float32 output (key-major; row k has
    the input batch's layout); `out_ragged(k)` views key k as a Ragged batch for the metric stage.  On the conv engine the padded
    copy and the forward product are computed once for the K keys."""

    def __init__(self, plan, ragged, cut_bins, out=None):
        _check_reflect(plan, ragged.lens_host)
        if ragged.data.dtype != torch.float32:
            raise ValueError("the STFT-domain low-pass takes float32 signals (torchlibrosa's convolution does too)")
        self.plan, self.r = plan, ragged
        self.rows = _Rows(plan, ragged.lens_host, ragged.device)
        self.cuts = np.asarray(cut_bins, dtype=np.int32).reshape(-1)
        self.n_keys = int(self.cuts.size)
        self.ws_bytes = int(plan.lib.ssr_ola_workspace_bytes(plan.handle, self.rows.total))
        self.ws = _workspace(self.ws_bytes, ragged.device)
        total = ragged.data.numel()
        if out is not None and (out.dtype != torch.float32 or out.numel() != self.n_keys * total or not out.is_contiguous()):
            raise ValueError("out must be a contiguous float32 buffer of n_keys x the batch's size")
        self.out = (out if out is not None else torch.empty(self.n_keys * total, dtype=torch.float32, device=ragged.device)).view(self.n_keys, total)

    def run(self):
        p, r = self.plan, self.r
        if r.n and self.n_keys:
            _lib.check(p.lib.ssr_fft_lowpass_multi(p.handle, _vp(r.data), _vp(r.off), _vp(r.len), self.cuts.ctypes.data_as(C.c_void_p),
                                                   self.n_keys, _vp(self.rows.off), r.n, r.max_len, self.rows.total, _vp(self.out),
                                                   r.data.numel(), _vp(self.ws), self.ws_bytes, _stream()))
        return self.out

    def out_ragged(self, k):
        return Ragged(self.out[k], self.r.off, self.r.len, self.r.lens_host)


def fft_lowpass_multi(plan, wavs, cut_bins):
    """K hard low-passes of every waveform of a list: [[key 0's outputs], [key 1's], ...]."""
    with torch.cuda.device(plan.device):
        r = wavs if isinstance(wavs, Ragged) else Ragged.from_list(wavs, plan.device)
        if r.n == 0:
            return [[] for _ in cut_bins]
        b = MultiLowpassBatch(plan, r, cut_bins)
        out = b.run()
        return [r.split(out[k]) for k in range(b.n_keys)]


def fft_lowpass(plan, wavs, cut_bins):
    """STFT-domain hard low-pass (K6) of a list of waveforms; cut_bins: first zeroed bin per item."""
    with torch.cuda.device(plan.device):
        r = wavs if isinstance(wavs, Ragged) else Ragged.from_list(wavs, plan.device)
        if r.n == 0:
            return []
        b = LowpassBatch(plan, r, cut_bins)
        return r.split(b.run())


def istft(plan, res, ims, lengths):
    """Inverse STFT (K6') of lists of [T_i, F] float32 (re, im); lengths: output samples per item."""
    with torch.cuda.device(plan.device):
        dev = plan.device
        lens = np.asarray(lengths, dtype=np.int64)
        if len(lens) == 0:
            return []
        _check_reflect(plan, lens)
        rows = _Rows(plan, lens, dev)
        for r_, t_ in zip(res, rows.T):
            if r_.shape[0] != t_ or r_.shape[1] != plan.n_bins:
                raise ValueError("spectrogram rows do not match ssr_num_frames(length)")
        re = torch.cat([r_.to(device=dev, dtype=torch.float32).reshape(-1) for r_ in res])
        im = torch.cat([i_.to(device=dev, dtype=torch.float32).reshape(-1) for i_ in ims])
        out_off = _offsets(lens)
        out = torch.empty(int(lens.sum()), dtype=torch.float32, device=dev)
        ws_bytes = int(plan.lib.ssr_ola_workspace_bytes(plan.handle, rows.total))
        ws = _workspace(ws_bytes, dev)
        # descriptor tensors must stay referenced until the launch has been enqueued: a temporary would be
        # returned to the caching allocator (and its block re-used by the next temporary) before the call
        lens_d = _h2d(lens.astype(np.int32), dev)
        out_off_d = _h2d(out_off, dev)
        _lib.check(plan.lib.ssr_istft(plan.handle, _vp(re), _vp(im), _vp(rows.off), _vp(lens_d), _vp(out_off_d), len(lens),
                                      int(lens.max()), rows.total, _vp(out), _vp(ws), ws_bytes, _stream()))
        return [out[out_off[i]:out_off[i] + lens[i]] for i in range(len(lens))]


# ------------------------------------------------------------------------------------------------------
class ResamplePlan:
    """Integer plan + taps of scipy.signal.resample_poly(x, up, down): float32 taps for a float32
    signal, the unrounded float64 design for a float64 one - as SciPy casts `h` to the signal's dtype."""

    _cache = {}

    def __init__(self, up, down, device):
        from scipy.signal import firwin  # tap design exactly as SciPy does it (host, once per rate pair)
        lib = _lib.load()
        u, d, n_out, hl, pp, pr = C.c_int(), C.c_int(), C.c_int64(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(lib.ssr_resample_plan(0, int(up), int(down), C.byref(u), C.byref(d), C.byref(n_out), C.byref(hl),
                                         C.byref(pp), C.byref(pr)))
        self.up, self.down, self.half_len = u.value, d.value, hl.value
        self.n_pre_pad, self.n_pre_remove = pp.value, pr.value
        self.identity = self.up == 1 and self.down == 1
        if self.identity:                      # scipy returns x.copy() before designing any filter
            self.taps_host, self.taps, self.taps64 = None, None, None
            return
        h64 = firwin(2 * self.half_len + 1, 1.0 / max(self.up, self.down), window=("kaiser", 5.0))
        h = h64.astype(np.float32)
        h *= self.up                            # scipy: h = h.astype(x.dtype) first, then h * up
        self.taps_host = np.concatenate((np.zeros(self.n_pre_pad, np.float32), h))
        self.taps = torch.from_numpy(self.taps_host).to(device)
        self.taps64 = torch.from_numpy(np.concatenate((np.zeros(self.n_pre_pad), h64 * self.up))).to(device)

    @classmethod
    def get(cls, up, down, device):
        g = math.gcd(int(up), int(down))
        key = (int(up) // g, int(down) // g, str(device))
        p = cls._cache.get(key)
        if p is None:
            p = cls._cache[key] = cls(up, down, device)
        return p

    def n_out(self, n_in):
        return -(-int(n_in) * self.up // self.down)


class ResampleBatch:
    """A ragged batch + cached output descriptors / buffer for repeated ssr_resample_poly calls (K7)."""

    def __init__(self, ragged, up, down, exact=True, alloc=True):
        dev = ragged.device
        self.r, self.rp = ragged, ResamplePlan.get(up, down, dev)
        self.exact = exact
        self.f64 = ragged.data.dtype == torch.float64
        if self.rp.identity:
            self.out_len = ragged.lens_host.copy()
        else:
            self.out_len = np.array([self.rp.n_out(n) for n in ragged.lens_host], dtype=np.int64)
        self.out_off = _offsets(self.out_len)
        self.out_off_d = _h2d(self.out_off, dev)
        self.out_len_d = _h2d(self.out_len.astype(np.int32), dev)
        self.out = torch.empty(int(self.out_len.sum()), dtype=ragged.data.dtype, device=dev) if alloc else None

    def run(self):
        r, rp = self.r, self.rp
        if self.out is None:
            self.out = torch.empty(int(self.out_len.sum()), dtype=r.data.dtype, device=r.device)
        if rp.identity:
            self.out.copy_(r.data)             # scipy returns x.copy() before designing any filter
        elif r.n and self.out_len.max() > 0:
            taps = rp.taps64 if self.f64 else rp.taps
            lib = _lib.load()
            args = (_vp(r.data), _vp(r.off), _vp(r.len), _vp(self.out_off_d), _vp(self.out_len_d), r.n,
                    int(self.out_len.max()), rp.up, rp.down, _vp(taps), int(taps.numel()), rp.n_pre_remove, _vp(self.out), _stream())
            # exact=False: the matrix-core kernel (float32 fused multiply-adds: within ~1 ulp per tap of SciPy's sums, not its
            # bits) where the plan fits it; float64 signals and plans it does not hold run the bit-exact kernel
            rc = _lib.ERR_UNSUPPORTED if (self.f64 or self.exact) else lib.ssr_resample_poly_mfma(*args)
            if rc == _lib.ERR_UNSUPPORTED:
                rc = (lib.ssr_resample_poly_f64 if self.f64 else lib.ssr_resample_poly)(*args)
            _lib.check(rc)
        return self.out

    def out_ragged(self):
        return Ragged(self.out, self.out_off_d, self.out_len_d, self.out_len)


class ResampleChainBatch:
    """resample_poly(resample_poly(x, mid, orig), new, mid) for a ragged float32 (or float64: two calls) batch - BASELINE cfg-5's 16 kHz -> 44.1 kHz -> 48 kHz.
    Where the two plans fit ssr_resample_poly_chain (21-tap phases, 8 up1 = 24 down2: 441/160 then 160/147) ONE kernel runs both
    stages and the intermediate signal never leaves LDS; otherwise the two stages run through ssr_resample_poly.  Same bits either
    way (SciPy's).  `fused`: None = try the fused kernel, False = always two calls."""

    def __init__(self, ragged, sr_orig, sr_mid, sr_new, fused=None):
        self.r = ragged
        self.s1 = ResampleBatch(ragged, sr_mid, sr_orig, alloc=False)
        mid = Ragged(torch.empty(0, dtype=ragged.data.dtype, device=ragged.device), self.s1.out_off_d, self.s1.out_len_d,
                     self.s1.out_len)                                          # geometry only: the buffer may never exist
        self.s2 = ResampleBatch(mid, sr_new, sr_mid, alloc=False)
        self.out_len, self.out_off, self.out_off_d, self.out_len_d = self.s2.out_len, self.s2.out_off, self.s2.out_off_d, self.s2.out_len_d
        # (a float64 batch runs the two stages in float64 - what SciPy does per dtype - and so is its output: ADVICE r4)
        self.out = torch.empty(int(self.out_len.sum()), dtype=ragged.data.dtype, device=ragged.device)
        self.s2.out = self.out
        self.fused = fused
        self.ran_fused = None
        if ragged.data.dtype != torch.float32 or self.s1.rp.identity or self.s2.rp.identity:
            self.fused = False

    def run(self):
        r, p1, p2 = self.r, self.s1.rp, self.s2.rp
        if self.fused is not False and r.n and self.out_len.max() > 0:
            rc = _lib.load().ssr_resample_poly_chain(
                _vp(r.data), _vp(r.off), _vp(r.len), _vp(self.s1.out_len_d), _vp(self.out_off_d), _vp(self.out_len_d), r.n,
                int(self.out_len.max()), p1.up, p1.down, _vp(p1.taps), int(p1.taps.numel()), p1.n_pre_remove,
                p2.up, p2.down, _vp(p2.taps), int(p2.taps.numel()), p2.n_pre_remove, _vp(self.out), _stream())
            if rc != _lib.ERR_UNSUPPORTED:
                _lib.check(rc)
                self.ran_fused = True
                return self.out
            if self.fused:
                _lib.check(rc)
        self.ran_fused = False
        self.run_stage1()
        return self.run_stage2()

    def run_stage1(self):
        """Stage 1 alone, into the intermediate buffer (allocated on first use)."""
        return self.s1.run()

    def run_stage2(self):
        """Stage 2 alone, from the intermediate buffer run_stage1() filled."""
        self.s2.r = self.s1.out_ragged()
        return self.s2.run()

    def out_ragged(self):
        return Ragged(self.out, self.out_off_d, self.out_len_d, self.out_len)


def resample_poly_chain(wavs, sr_orig, sr_mid, sr_new, device=None, fused=None):
    """scipy.signal.resample_poly twice (sr_orig -> sr_mid -> sr_new) for a list of float32 waveforms; see ResampleChainBatch."""
    dev = torch.device(device) if device is not None else default_device()
    with torch.cuda.device(dev):
        r = wavs if isinstance(wavs, Ragged) else Ragged.from_list(wavs, dev)
        b = ResampleChainBatch(r, sr_orig, sr_mid, sr_new, fused=fused)
        out = b.run()
        return [out[b.out_off[i]:b.out_off[i] + b.out_len[i]] for i in range(r.n)]


def resample_poly(wavs, up, down, device=None, exact=True):
    """Polyphase resampling (K7) of a list of waveforms; bit-identical to scipy.signal.resample_poly.  A batch
    holding float64 signals is resampled in float64 (float64 taps and accumulation), everything else in float32.
    exact=False: float32 signals go through the matrix-core kernel (ssr_resample_poly_mfma: the same sums with fused
    multiply-adds, ~1 ulp per tap from SciPy's values, 1.2-1.5x the rate)."""
    dev = torch.device(device) if device is not None else default_device()
    with torch.cuda.device(dev):
        # views into ONE device buffer in increasing address order are read where they lie (the kernels take an offset per signal):
        # the IIR keys of a batch - [design][file] slices of ssr_sosfiltfilt_multi's output - used to be concatenated again here
        # (11 GB and 13 k per-signal calls per evaluate() batch of 256 files x 36 keys)
        r = wavs if isinstance(wavs, Ragged) else Ragged.from_list_keep64(wavs, dev, allow_gaps=True)
        if not r.packed and ResamplePlan.get(up, down, dev).identity:
            r = Ragged.from_list_keep64(wavs, dev)              # (the identity plan copies the packed buffer)
        b = ResampleBatch(r, up, down, exact=exact)
        out = b.run()
        return [out[b.out_off[i]:b.out_off[i] + b.out_len[i]] for i in range(r.n)]


# ------------------------------------------------------------------------------------------------------
_SINC_FILTERS = {  # resampy filter name -> (num_zeros, precision, Kaiser beta, roll-off)   (resampy/filters.py)
    "kaiser_best": (64, 9, 14.769656459379492, 0.9475937167399596),
    "kaiser_fast": (16, 9, 8.555504641634386, 0.85),
}


class SincPlan:
    """Interpolation tables of resampy.resample(x, sr_orig, sr_new, filter=name) on the device (N2): the right half of
    the Kaiser-windowed sinc, regenerated from the filter's documented parameters on the host in float64 (a plan, like
    the polyphase taps), its forward differences, and the running time register t_k = fl(t_{k-1} + 1/ratio)."""

    _cache = {}

    def __init__(self, sr_orig, sr_new, name, device):
        from scipy.signal.windows import kaiser
        if name not in _SINC_FILTERS:
            raise NotImplementedError("resampling filter %r (supported: %s)" % (name, sorted(_SINC_FILTERS)))
        nz, prec, beta, roll = _SINC_FILTERS[name]
        self.ratio = float(sr_new) / float(sr_orig)
        # filter phases repeat every `a` outputs when sr_new / sr_orig = a / b in lowest terms (a work-mapping hint)
        self.phase_period = 0
        if float(sr_new).is_integer() and float(sr_orig).is_integer():
            self.phase_period = int(sr_new) // math.gcd(int(sr_new), int(sr_orig))
        self.num_table = 2 ** prec
        n = self.num_table * nz
        win = kaiser(2 * n + 1, beta)[n:] * (roll * np.sinc(roll * np.linspace(0, nz, num=n + 1, endpoint=True)))
        if self.ratio < 1:
            win = win * self.ratio
        delta = np.zeros_like(win)
        delta[:-1] = np.diff(win)
        self.scale = min(1.0, self.ratio)
        self.index_step = int(self.scale * self.num_table)
        self.n_win = int(win.shape[0])
        self.device = device
        self.win = torch.from_numpy(win).to(device)
        self.delta = torch.from_numpy(delta).to(device)
        self._tr, self._tr_len = None, 0

    @classmethod
    def get(cls, sr_orig, sr_new, name, device):
        key = (float(sr_orig), float(sr_new), name, str(device))
        p = cls._cache.get(key)
        if p is None:
            p = cls._cache[key] = cls(sr_orig, sr_new, name, device)
        return p

    def n_out(self, n_in):
        return int(int(n_in) * self.ratio)                      # resampy: int(shape * sample_ratio)

    def time_register(self, n):
        """Device float64 [>= n]: resampy's `time_register += time_increment`, a SEQUENTIAL float64 sum (np.cumsum)."""
        if n > self._tr_len:
            m = max(n, 2 * self._tr_len, 1 << 16)
            tr = np.empty(m)
            tr[0] = 0.0
            tr[1:] = np.cumsum(np.full(m - 1, 1.0 / self.ratio))
            self._tr, self._tr_len = torch.from_numpy(tr).to(self.device), m
        return self._tr


def resample_sinc(wavs, sr_orig, sr_new, res_type="kaiser_best", device=None, fix=True):
    """librosa.resample(y, sr_orig, sr_new, res_type="kaiser_best" | "kaiser_fast") for a list of float32 waveforms (N2):
    resampy's band-limited interpolation on the GPU, then librosa's fix_length to ceil(n * ratio).  Device tensors out."""
    dev = torch.device(device) if device is not None else default_device()
    with torch.cuda.device(dev):
        r = wavs if isinstance(wavs, Ragged) else Ragged.from_list(wavs, dev)
        if float(sr_orig) == float(sr_new):
            return [w.clone() for w in r.split()]
        sp = SincPlan.get(sr_orig, sr_new, res_type, dev)
        out_len = np.array([sp.n_out(n) for n in r.lens_host], dtype=np.int64)
        want = np.array([int(np.ceil(n * sp.ratio)) for n in r.lens_host], dtype=np.int64) if fix else out_len
        out_off = _offsets(want)
        out = torch.zeros(int(want.sum()), dtype=torch.float32, device=dev)       # fix_length pads with zeros
        if r.n and out_len.max() > 0:
            out_off_d = _h2d(out_off, dev)
            out_len_d = _h2d(out_len.astype(np.int32), dev)
            tr = sp.time_register(int(out_len.max()))
            _lib.check(_lib.load().ssr_resample_sinc(_vp(r.data), _vp(r.off), _vp(r.len), _vp(out_off_d), _vp(out_len_d), r.n,
                                                     int(out_len.max()), _vp(tr), int(tr.numel()), _vp(sp.win), _vp(sp.delta),
                                                     sp.n_win, sp.num_table, sp.index_step, float(sp.scale), float(sp.ratio),
                                                     int(sp.phase_period), _vp(out), _stream()))
        return [out[out_off[i]:out_off[i] + want[i]] for i in range(r.n)]


class _Staging:
    """Two page-locked int16 arenas per device, used alternately: a batch's PCM is packed into one of them and crosses PCIe in
    ONE asynchronous copy while the host packs the next batch into the other.  An arena is reused only after the copy that
    last read it has completed (event)."""
    _by_dev = {}
    _by_dev_lock = threading.Lock()

    def __init__(self):
        self.buf = [None, None]
        self.ev = [None, None]
        self.twin = [None, None]                # the arenas' device-side twins and the events behind their last readers (_h2d_arena)
        self.done = [None, None]
        self.k = 0
        self.lock = threading.Lock()

    @classmethod
    def get(cls, dev, role="packed"):
        """One arena pair per (resolved device index, role).  role "packed": io.PackedBatch (the prefetching file path);
        "list": upload_decoded() of a list of RawAudio - its own pair, so that a list upload in the middle of an in-flight
        PackedBatch (its non-RIFF `others`) can never flip that batch's arenas."""
        idx = _device_index(torch.device(dev))
        with cls._by_dev_lock:
            return cls._by_dev.setdefault((idx, role), cls())

    def arena(self, n):
        with self.lock:
            self.k ^= 1
            k = self.k
            ev = self.ev[k]
        if ev is not None:
            ev.synchronize()
        with self.lock:
            if self.buf[k] is None or self.buf[k].numel() < n:
                self.buf[k] = torch.empty(max(n, 1 << 22), dtype=torch.int16, pin_memory=True)
            return k, self.buf[k]

    def sent(self, k):
        ev = torch.cuda.Event()
        ev.record()
        with self.lock:
            self.ev[k] = ev


_upload_streams = {}


def _h2d_arena(st, k, arena, total, dev):
    """Page-locked int16 arena k of staging pair `st` -> its device twin, on the device's UPLOAD stream: the bus transfer of a batch
    runs under the kernels of the batch before it instead of queueing behind them (6 ms of an evaluate() pass over 367 files).  The
    twin is a persistent buffer (grown when a batch needs more), so no allocation crosses the two streams' pools.  Ordering, all on
    the GPU: the upload stream waits for the event recorded behind the last kernel that read the twin (consumed()), the current
    stream waits for the copy.  -> (the twin's first `total` elements, consumed)."""
    idx = _device_index(dev)
    side = _upload_streams.get(idx)
    if side is None:
        side = _upload_streams[idx] = torch.cuda.Stream(device=idx)
    cur = torch.cuda.current_stream(idx)
    with st.lock:
        twin, done = st.twin[k], st.done[k]
    if twin is None or twin.numel() < total or twin.device.index != idx:
        twin = torch.empty(max(total, 1 << 22), dtype=torch.int16, device=dev)       # (its old self is freed stream-ordered, on `cur`)
        side.wait_stream(cur)
    if done is not None:
        side.wait_event(done)
    with torch.cuda.stream(side):
        twin[:total].copy_(arena[:total], non_blocking=True)
        st.sent(k)
    cur.wait_stream(side)

    def consumed():
        ev = torch.cuda.Event()
        ev.record(cur)
        with st.lock:
            st.twin[k], st.done[k] = twin, ev
    return twin[:total], consumed


def _pcm_to_float(d16, in_off, frames, chans, dev):
    """int16 device buffer + host descriptors -> (flat float32 mono device buffer, host out offsets)."""
    n = len(frames)
    out_off = _offsets(frames)
    desc = _h2d(np.concatenate((in_off, out_off)).astype(np.int64), dev)
    desc32 = _h2d(np.concatenate((frames.astype(np.int32), chans.astype(np.int32))), dev)
    flat = torch.empty(int(frames.sum()), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().ssr_pcm16_to_float(_vp(d16), _vp(desc[:n]), _vp(desc32[:n]), _vp(desc32[n:]), n, int(frames.max()),
                                              _vp(flat), _vp(desc[n:]), _stream()))
    return flat, out_off


def upload_decoded(raw, device=None):
    """Decoded files -> float32 mono device tensors, one per file.  `raw`: an io.PackedBatch (the files' PCM already sits in a
    page-locked arena) or a list of io.RawAudio.  16-bit PCM crosses the bus as int16 - half the bytes, no float pass on the
    host - in one pinned asynchronous copy per batch and is converted / mixed to mono on the GPU (ssr_pcm16_to_float);
    anything else is uploaded as the float32 mono array it already is."""
    from .io import PackedBatch
    if isinstance(raw, PackedBatch):
        dev = torch.device(raw.device)
        out = [None] * len(raw.paths)
        with torch.cuda.device(dev):
            if raw.total:                      # the arena's copy (and its event) first: nothing else touches this batch's arena
                d16, consumed = _h2d_arena(raw.staging, raw.k, raw.arena, raw.total, dev)
                flat, out_off = _pcm_to_float(d16, raw.in_off, raw.frames, raw.chans, dev)
                consumed()
                for j, i in enumerate(raw.pcm_idx):
                    out[i] = flat[out_off[j]:out_off[j] + raw.frames[j]]
            for i, r in zip(raw.other_idx, raw.others):           # (these go through the "list" arenas, a separate pair)
                out[i] = upload_decoded([r], dev)[0]
        return out
    dev = torch.device(device) if device is not None else default_device()
    out = [None] * len(raw)
    with torch.cuda.device(dev):
        pcm = [i for i, r in enumerate(raw) if r.pcm is not None and r.pcm.shape[0] > 0]
        is_pcm = set(pcm)
        for i, r in enumerate(raw):
            if i not in is_pcm:
                out[i] = torch.from_numpy(np.ascontiguousarray(r.to_float(), dtype=np.float32)).to(dev, non_blocking=True)
        if pcm:
            sizes = np.array([raw[i].pcm.shape[0] for i in pcm], dtype=np.int64)
            frames = np.array([raw[i].n_frames for i in pcm], dtype=np.int64)
            chans = np.array([raw[i].nch for i in pcm], dtype=np.int32)
            total = int(sizes.sum())
            st = _Staging.get(dev, "list")
            k, arena = st.arena(total)
            host = arena.numpy()
            in_off = _offsets(sizes)
            for i, o in zip(pcm, in_off):
                host[o:o + raw[i].pcm.shape[0]] = raw[i].pcm
            d16, consumed = _h2d_arena(st, k, arena, total, dev)
            flat, out_off = _pcm_to_float(d16, in_off, frames, chans, dev)
            consumed()
            for j, i in enumerate(pcm):
                out[i] = flat[out_off[j]:out_off[j] + frames[j]]
    return out


def sosfiltfilt(sos, wavs, device=None, exact=True):
    """scipy.signal.sosfiltfilt(sos, x) for a list of float32 (or float64) waveforms on the GPU (N1); float64 tensors out.
    The section coefficients and sosfilt_zi come from SciPy on the host (filter design, as in the reference).
    exact=True: SciPy's bits.  exact=False: the segment-parallel kernel (ssr_sosfiltfilt_fast: the same filter evaluated parallel in
    time, within 1e-10 of each signal's peak of SciPy's result, not its bits; the same bits as this design's slot of
    sosfiltfilt_multi(exact=False)); a design of more than 8 sections takes the exact kernel whatever `exact` says."""
    from scipy.signal import sosfilt_zi
    if not exact and np.ndim(sos) == 2 and np.shape(sos)[0] <= SOS_FAST_MAX_SECTIONS:
        return sosfiltfilt_multi([sos], wavs, device, exact=False)[0]
    dev = torch.device(device) if device is not None else default_device()
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError("sos must have shape (n_sections, 6)")
    n_sections = sos.shape[0]
    edge = _sos_edge(sos)
    with torch.cuda.device(dev):
        r = wavs if isinstance(wavs, Ragged) else Ragged.from_list_keep64(wavs, dev)
        if r.n == 0:
            return []
        if int(r.lens_host.min()) <= edge:
            raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % edge)
        lib = _lib.load()
        total = int(r.lens_host.sum())
        sos_d = _h2d(sos, dev)
        zi_d = _h2d(np.ascontiguousarray(sosfilt_zi(sos), dtype=np.float64), dev)
        ws_bytes = int(lib.ssr_sosfiltfilt_workspace_bytes(total, r.n, edge))
        ws = _workspace(ws_bytes, dev)
        y = torch.empty(total, dtype=torch.float64, device=dev)
        fn = lib.ssr_sosfiltfilt_f64 if r.data.dtype == torch.float64 else lib.ssr_sosfiltfilt
        _lib.check(fn(_vp(r.data), _vp(r.off), _vp(r.len), r.n, total, _vp(sos_d), _vp(zi_d), n_sections, edge, _vp(y), _vp(ws),
                      ws_bytes, _stream()))
        return r.split(y)


def _sos_edge(sos):
    n_sections = sos.shape[0]
    ntaps = 2 * n_sections + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
    return 3 * ntaps


SOS_FAST_MAX_SECTIONS = 8                                        # ssr_sosfiltfilt_fast's limit
SOS_MULTI_MAX_DESIGNS = 48                                       # designs per launch (the C ABI's limit)
# Output doubles per launch.  A launch lasts as long as its LONGEST utterance (a serial recurrence, ~195 cycles per sample step) whatever
# the number of (design, utterance) recurrences beside it, until the chip's wave slots are full (4 recurrences per wave, ~2.5 waves per
# SIMD by LDS): 64 files x 36 designs are 576 waves on 1024 SIMDs.  16 GiB of output per launch (round 6; 4 GiB before) lets a batch of
# 256 files x 36 designs go in ONE launch - evaluate() with 36 IIR keys 0.94 -> 0.74 s per 367 files; sosfiltfilt_multi also keeps
# the launch inside a quarter of the device's free memory.
SOS_MULTI_MAX_DOUBLES = int(os.environ.get("SSR_SOS_MULTI_MAX_DOUBLES", 1 << 31))


def sosfiltfilt_multi(sos_list, wavs, device=None, exact=True):
    """scipy.signal.sosfiltfilt(sos, x) for EVERY design of sos_list over one list of float32 waveforms: ssr_sosfiltfilt_multi, the
    designs side by side in one launch (a launch is latency-bound - the recurrence is serial in time - and fills an eighth of a wave
    per utterance: one design after the other costs the same latency each time).  -> [design][signal] float64 device tensors, every one
    bit-identical to sosfiltfilt(sos, ...).  Designs of more than 8 sections and float64 signals go through sosfiltfilt().
    exact=False: ssr_sosfiltfilt_fast / _f64 instead - every design evaluated parallel in time (segments of the signal side by side,
    their states handed on by a short scan), float32 and float64 signals alike, designs chunked per launch the same way.  The
    result is within 1e-10 of each signal's peak of SciPy's, NOT its bits; it is deterministic and does not depend on what a signal
    is batched with.  A design of more than 8 sections (a band-pass of order > 8) falls back to the exact kernel - the only
    fallback: a Ragged of views with gaps (not `packed`) raises ValueError."""
    dev = torch.device(device) if device is not None else default_device()
    sos_list = [np.ascontiguousarray(s_, dtype=np.float64) for s_ in sos_list]
    for s_ in sos_list:
        if s_.ndim != 2 or s_.shape[1] != 6:
            raise ValueError("sos must have shape (n_sections, 6)")
    if not sos_list:                   # no design: no keys (the reference's nested loops run zero times, ssr_eval/eval.py:243-258)
        return []
    with torch.cuda.device(dev):
        r = wavs if isinstance(wavs, Ragged) else Ragged.from_list_keep64(wavs, dev)
        if r.n == 0:
            return [[] for _ in sos_list]
        if not exact:
            if not r.packed:           # (the exact path refuses it too, in split(); here before anything runs, not by another kernel)
                raise ValueError("a batch of views with gaps has no packed layout to split")
            small = [k for k, s_ in enumerate(sos_list) if s_.shape[0] <= SOS_FAST_MAX_SECTIONS]
            out = [None] * len(sos_list)
            for k, ys in zip(small, _sosfiltfilt_fast([sos_list[k] for k in small], r, dev)):
                out[k] = ys
            return [ys if ys is not None else sosfiltfilt(s_, r, dev) for s_, ys in zip(sos_list, out)]
        if r.data.dtype != torch.float32 or any(s_.shape[0] > 8 for s_ in sos_list) or not r.packed:
            return [sosfiltfilt(s_, r if r.packed else wavs, dev) for s_ in sos_list]
        edges = [_sos_edge(s_) for s_ in sos_list]
        if int(r.lens_host.min()) <= max(edges):
            raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % max(edges))
        return _sosfiltfilt_launches(sos_list, edges, r, dev, "ssr_sosfiltfilt_multi_workspace_bytes", "ssr_sosfiltfilt_multi")


def _sosfiltfilt_launches(sos_list, edges, r, dev, ws_name, fn_name):
    """The designs of sos_list (<= 8 sections each) over the packed batch r, SOS_MULTI_MAX_DESIGNS and SOS_MULTI_MAX_DOUBLES output
    doubles per launch at most, through one of the multi-design entry points -> [design][signal]."""
    from scipy.signal import sosfilt_zi
    lib = _lib.load()
    ws_fn, fn = getattr(lib, ws_name), getattr(lib, fn_name)
    total = int(r.lens_host.sum())
    try:
        free_doubles = int(torch.cuda.mem_get_info(dev)[0]) // 8 // 4
    except Exception:
        free_doubles = SOS_MULTI_MAX_DOUBLES
    per_launch = max(1, min(SOS_MULTI_MAX_DESIGNS, min(SOS_MULTI_MAX_DOUBLES, free_doubles) // max(total, 1)))
    out = []
    for d0 in range(0, len(sos_list), per_launch):
        chunk = sos_list[d0:d0 + per_launch]
        D = len(chunk)
        sos_h, zi_h = np.zeros((D, 8, 6)), np.zeros((D, 8, 2))
        for d, s_ in enumerate(chunk):
            sos_h[d, :s_.shape[0]] = s_
            zi_h[d, :s_.shape[0]] = sosfilt_zi(s_)
        ns = np.array([s_.shape[0] for s_ in chunk], dtype=np.int32)
        eg = np.array(edges[d0:d0 + D], dtype=np.int32)
        sos_d, zi_d = _h2d(sos_h, dev), _h2d(zi_h, dev)
        ws_bytes = int(ws_fn(total, r.n, eg.ctypes.data_as(C.c_void_p), D))
        ws = _workspace(ws_bytes, dev)
        y = torch.empty((D, total), dtype=torch.float64, device=dev)
        _lib.check(fn(_vp(r.data), _vp(r.off), _vp(r.len), r.n, total, _vp(sos_d), _vp(zi_d), ns.ctypes.data_as(C.c_void_p),
                      eg.ctypes.data_as(C.c_void_p), D, _vp(y), total, _vp(ws), ws_bytes, _stream()))
        out += [r.split(y[d]) for d in range(D)]
    return out


def _sosfiltfilt_fast(sos_list, r, dev):
    """sosfiltfilt_multi(exact=False) for designs of <= 8 sections over a packed float32 or float64 batch."""
    if not sos_list:
        return []
    edges = [_sos_edge(s_) for s_ in sos_list]
    if int(r.lens_host.min()) <= max(edges):
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % max(edges))
    f64 = r.data.dtype == torch.float64
    return _sosfiltfilt_launches(sos_list, edges, r, dev, "ssr_sosfiltfilt_fast_workspace_bytes",
                                 "ssr_sosfiltfilt_fast_f64" if f64 else "ssr_sosfiltfilt_fast")


def xcorr_argmax(a_list, b_list, device=None):
    """numpy.argmax(scipy.signal.correlate(a, b, "full")) for lists of equal-length float32 signal pairs (N4)."""
    dev = torch.device(device) if device is not None else default_device()
    with torch.cuda.device(dev):
        ra, rb = Ragged.from_list(a_list, dev), Ragged.from_list(b_list, dev)
        if ra.n != rb.n or not np.array_equal(ra.lens_host, rb.lens_host):
            raise ValueError("cross-correlation alignment needs pairs of equal length (unify_length first)")
        if ra.n == 0:
            return np.zeros(0, np.int64)
        if int(ra.lens_host.min()) < 1:
            raise ValueError("empty signal")
        lib = _lib.load()
        ws_bytes = int(lib.ssr_xcorr_workspace_bytes(ra.n, ra.max_len))
        ws = _workspace(ws_bytes, dev)
        out = torch.empty(ra.n, dtype=torch.int64, device=dev)
        _lib.check(lib.ssr_xcorr_argmax(_vp(ra.data), _vp(ra.off), _vp(rb.data), _vp(rb.off), _vp(ra.len), ra.n, ra.max_len,
                                        _vp(out), _vp(ws), ws_bytes, _stream()))
        return out.cpu().numpy()
