"""Destriping map-maker on MI355X (drop-in for comancpipeline/MapMaking/Destriper.py).

``run_destriper`` keeps the reference signature and return value
(Destriper.py:456-503): ``{'All': {'map', 'naive', 'weight', 'map2', 'hits'}}``
on rank 0 and ``None`` maps on other ranks.  Internally:

* ``DeviceOps`` -- one rank's samples as the constant offset<->pixel sparse
  operator built by ``comap_destripe_create`` (csrc/destriper_setup.hip);
* ``cg_solve`` -- the reference BiCG (Destriper.py:85-152) with its two
  duplicate matvecs folded (p == pb, r == rb), run on device vectors; per
  iteration the only exchange is a SUM all-reduce of the map numerator
  (npix f64) and of two scalars (p.q, r.r) -- RCCL over xGMI when
  torch.distributed is initialised with the nccl backend.  ``cg_solve`` is
  backend-agnostic (the gloo CPU tests drive it with the oracle's NumPy ops).

Samples are sharded by whole offsets (the reference shards files,
run_destriper.py:131-138); the map is replicated.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from .. import _native as N


def _dist():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist
    except ImportError:  # pragma: no cover
        pass
    return None


def torch_allreduce(t):
    """SUM all-reduce in place (no-op on one rank)."""
    d = _dist()
    if d is not None and d.get_world_size() > 1:
        d.all_reduce(t, op=d.ReduceOp.SUM)
    return t


def _device(device):
    """torch's device object of HIP device ``device`` (None: the current one)."""
    import torch
    return torch.device('cuda', N.current_device() if device is None else int(device))


def _to_tensor(a, dev, dt):
    """Array or tensor as a tensor of dtype ``dt`` on ``dev``."""
    import torch
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dt)


def lane_tree_sum(v):
    """The sum of ``v`` in the residual pass's lane-tree order (comap_destripe_residuals), in
    NumPy: lane l of 64 adds v[l], v[l + 64], v[l + 128], ... in that order from +0.0; then for
    s = 32, 16, 8, 4, 2, 1: a[l] = a[l] + a[l ^ s]; the result is lane 0's.  I.e. ``v`` padded
    with +0.0 to a multiple of 64 as [K, 64], its rows added in order, then folded."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    rows = np.zeros((-(-v.size // 64), 64))
    rows.reshape(-1)[:v.size] = v
    a = np.zeros(64)
    for row in rows:
        a = a + row
    for s in (32, 16, 8, 4, 2, 1):
        a = a[:s] + a[s:2 * s]
    return float(a[0])


def _prior_runs(gid, n_groups):
    """(s, e) int64 [n_groups]: the one run [s_g, e_g) of offsets every noise-prior group id
    occupies (0, 0 for a group without offsets).  ValueError for an id outside [-1, n_groups) or
    a group in more than one run."""
    gid = np.asarray(gid).reshape(-1).astype(np.int64)
    G = int(n_groups)
    if gid.size and (gid.min() < -1 or gid.max() >= G):
        raise ValueError(f'noise prior: group id out of range (valid: -1 .. {G - 1})')
    first = np.nonzero(np.concatenate([[True], gid[1:] != gid[:-1]]) & (gid >= 0))[0] if gid.size else np.zeros(0, int)
    last = np.nonzero(np.concatenate([gid[1:] != gid[:-1], [True]]) & (gid >= 0))[0] if gid.size else np.zeros(0, int)
    if np.unique(gid[first]).size != first.size:
        raise ValueError('noise prior: a group id occupies more than one run of offsets')
    s, e = np.zeros(G, np.int64), np.zeros(G, np.int64)
    s[gid[first]], e[gid[last]] = first, last + 1
    return s, e


def prior_apply_reference(v, gid, stencil):
    """y = T v of the noise prior (comap_destripe_prior_apply) in NumPy, bit for bit: ``v`` f64 [n]
    and ``gid`` [n] in the caller's offset order, ``stencil`` f64 [G, K + 1].  Group g occupies the
    run [s_g, e_g); y_i = t_g[0] v_i, then for k = 1 .. K in this order y_i += t_g[k] v_{i-k} if
    i - k >= s_g and y_i += t_g[k] v_{i+k} if i + k < e_g, every product and sum rounded to f64 on
    its own; y_i = +0.0 where gid is -1.  ValueError for an id outside [-1, G) or a group in more
    than one run."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    gid = np.asarray(gid).reshape(-1).astype(np.int64)
    t = np.asarray(stencil, dtype=np.float64)
    if t.ndim != 2 or not 1 <= t.shape[1] - 1 <= 64:
        raise ValueError('noise prior: stencil must be [n_groups, K + 1] with 1 <= K <= 64')
    if gid.size != v.size:
        raise ValueError('noise prior: one group id per offset')
    s, e = _prior_runs(gid, t.shape[0])
    has = gid >= 0
    g = np.where(has, gid, 0)
    si, ei, i = s[g], e[g], np.arange(v.size)
    y = t[g, 0] * v
    for k in range(1, t.shape[1]):
        tk = t[g, k]
        m = has & (i - k >= si)
        y[m] = y[m] + tk[m] * v[i[m] - k]
        m = has & (i + k < ei)
        y[m] = y[m] + tk[m] * v[i[m] + k]
    y[~has] = 0.0
    return y


def noise_prior_stencil(fknee, alpha, L, fs=50.0, taps=16, M=4096):
    """The noise prior's stencil t[0 .. taps] for unit white variance: the inverse spectrum of the
    L-sample means of correlated noise P_c(f) = (fknee / f)^(-alpha) (alpha < 0), sampled at fs.

    For nu_j = j / M: P_a(nu) = (1/L) sum_{m<L} P_c(fs fold(phi_m)) D(phi_m), phi_m = (nu + m) / L,
    fold(phi) = min(phi, 1 - phi), D(phi) = (sin(pi phi L) / (L sin(pi phi)))^2 with D(0) = 1 -- the
    exact spectrum of the means, aliases included; P_c(0) = +inf, so 1 / P_a(0) = 0.
    t[k] = (1 - k / (taps + 1)) (1/M) sum_j cos(2 pi j k / M) / P_a(nu_j): the triangular taper
    convolves the symbol with a Fejer kernel, so it stays >= 0 and every finite section is positive
    semi-definite, at the price of a weak zero-mean prior per group (a non-zero row sum)."""
    K, L, M = int(taps), int(L), int(M)
    if not 1 <= K <= 64:
        raise ValueError(f'noise prior: taps must lie in 1 .. 64, not {taps}')
    if not (np.isfinite(fknee) and fknee > 0 and np.isfinite(alpha) and alpha < 0):
        raise ValueError(f'noise prior: needs fknee > 0 and alpha < 0, not {fknee}, {alpha}')
    if L < 1 or M <= 2 * K:
        raise ValueError('noise prior: needs L >= 1 and M > 2 taps')
    phi = (np.arange(M)[:, None] / M + np.arange(L)[None, :]) / L
    with np.errstate(divide='ignore', invalid='ignore'):
        f = fs * np.minimum(phi, 1.0 - phi)
        pc = np.where(f > 0, (fknee / np.where(f > 0, f, 1.0)) ** (-alpha), np.inf)
        sn = np.sin(np.pi * phi)
        D = np.where(sn != 0, (np.sin(np.pi * phi * L) / (L * np.where(sn != 0, sn, 1.0))) ** 2, 1.0)
        pa = (pc * D).sum(axis=1) / L
        inv = np.where(np.isfinite(pa) & (pa > 0), 1.0 / pa, 0.0)
    k = np.arange(K + 1)
    t = (np.cos(2 * np.pi * np.outer(k, np.arange(M)) / M) * inv[None, :]).sum(axis=1) / M
    return (1.0 - k / (K + 1.0)) * t


def fknee_from_red_noise(sigma_w, sigma_r, alpha):
    """The knee frequency (Hz) of a ``red_noise_model`` fit sigma_w^2 + sigma_r^2 f^alpha:
    (sigma_r / sigma_w)^(2 / |alpha|).  NaN (an invalid fit: the group gets no prior) unless
    sigma_w > 0, sigma_r > 0, alpha < 0 and all three are finite.  Scalars or arrays."""
    sw, sr, a = (np.asarray(v, dtype=np.float64) for v in (sigma_w, sigma_r, alpha))
    sw, sr, a = np.broadcast_arrays(sw, sr, a)
    ok = np.isfinite(sw) & np.isfinite(sr) & np.isfinite(a) & (sw > 0) & (sr > 0) & (a < 0)
    out = np.full(ok.shape, np.nan)
    out[ok] = (sr[ok] / sw[ok]) ** (2.0 / np.abs(a[ok]))
    return out if out.ndim else float(out)


class TimedAllreduce:
    """torch_allreduce with every call bracketed by HIP events on the current stream (the
    stream the CG kernels run on, which waits for the collective): the measured
    all-reduce time and bytes per CG iteration that mapmaking/rankplan.py's alpha / beta
    are calibrated from (bench.py, N > 1).  The first ``skip`` calls (the set-up sums of
    h, the naive numerator and rr0 in cg_solve_batched) are recorded apart."""

    def __init__(self, skip=3):
        self.calls, self.skip = [], skip

    def __call__(self, t):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_allreduce(t)
        e1.record()
        self.calls.append((t.numel() * t.element_size(), e0, e1))
        return t

    def summary(self, iterations):
        import torch
        torch.cuda.synchronize()
        body = self.calls[self.skip:]
        ms = [a.elapsed_time(b) for _, a, b in body]
        it = max(int(iterations), 1)
        per = len(body) // it if body else 0
        sizes = [n for n, _, _ in body[:per]]
        by_call = [sum(ms[k::per]) / it for k in range(per)] if per else []
        return {'iterations': it, 'calls_per_iter': per, 'bytes_per_call': sizes,
                'ms_per_call': by_call, 'allreduce_ms_per_iter': sum(ms) / it,
                'bytes_per_iter': sum(sizes)}


def compact_pixels(pix, npix, allreduce):
    """(pixel ids relabelled onto the union over ranks of the pixels the operator touches,
    int32; the union's pixel ids, increasing).  The union holds every binned pixel and
    every pixel an unbinned sample reads: op_Z reads m[pointing] (Destriper.py:206-213),
    so a negative id p reads pixel npix + p.  Such a sample keeps a negative id in the
    compacted map of nc pixels, cid[npix + p] - nc, which reads the same pixel there.
    pix: int64 torch tensor on any device (ids in [-npix, npix)); allreduce sums in place."""
    import torch
    read = torch.remainder(pix, npix)            # the pixel each sample bins or reads
    hit = torch.zeros(npix, dtype=torch.int32, device=pix.device)
    hit[read] = 1
    allreduce(hit)
    keep = hit > 0
    cid = torch.cumsum(keep.to(torch.int64), 0) - 1
    nc = int(keep.sum().item())
    comp = torch.where(pix >= 0, cid[read], cid[read] - nc)
    return comp.to(torch.int32), torch.nonzero(keep).reshape(-1)


def cg_solve(ops, allreduce, threshold=1e-6, niter=100, h=None, nnum=None):
    """Distributed CG for the destriper offsets.

    ops: operator object (DeviceOps or oracle.destriper.ShardOps) for this
    rank's samples; allreduce(array) sums in place across ranks.  h / nnum
    are the global weight map and naive numerator (computed when None).
    Returns (x, iterations, h, nnum); for DeviceOps x is in the problem's internal
    offset order (DeviceOps.natural converts)."""
    if getattr(ops, 'nb', 1) != 1:
        raise ValueError('cg_solve drives one band; batched bands use cg_solve_batched')
    if h is None or nnum is None:
        h0, _, n0 = ops.local_maps()
        h = allreduce(h0)
        nnum = allreduce(n0)
    NO = ops.n_offsets
    x = ops.zeros(NO)
    r = ops.zeros(NO)
    ops.project(None, nnum, h, r)                # b = op_Ax(tod, extend=False); r0 = b - A 0
    p = ops.copy(r)
    rr0 = ops.scalar()
    ops.dot(r, r, rr0)
    allreduce(rr0)
    rr = ops.copy(rr0)
    thresh0 = ops.host_scalar(rr0)
    num = ops.zeros(ops.npix)
    q = ops.zeros(NO)
    pq = ops.scalar()
    rrn = ops.scalar()
    it = 0
    for i in range(niter):
        ops.bin(p, 0, num)
        allreduce(num)
        ops.project(p, num, h, q, pq)
        allreduce(pq)
        ops.cg_update(rr, pq, x, r, p, q, rrn)
        allreduce(rrn)
        ops.cg_direction(rrn, rr, p, r)
        ops.set_scalar(rr, rrn)
        it = i + 1
        with np.errstate(divide='ignore', invalid='ignore'):    # b = 0: NaN (0 / 0) stops, as on the device
            delta = np.float64(ops.host_scalar(rrn)) / np.float64(thresh0)
        if np.isnan(delta) or delta < threshold:
            break
    return x, it, h, nnum


def cg_solve_batched(ops, allreduce, threshold=1e-6, niter=100, batch=16):
    """Multi-rank CG of the device path: the iterates of ``cg_solve`` (same
    order of operations and cross-rank sums), but with the convergence test on
    the device (the direction call's stop flags) so ``batch`` iterations --
    kernels and all-reduces -- are queued per host round trip.  Iterations
    queued after convergence are no-ops (their all-reduces sum stale buffers
    that are not read again).  ``ops`` is a DeviceOps -- every band of a batched
    problem at once (vectors interleaved [n][nb], one all-reduce per sum for
    all bands) -- or a GroundOps (nb = 1, vectors [x | s | c]; the iterates of
    ``cg_solve`` bit for bit, as each rank holds whole (observation, feed)
    groups).  Returns (x in the problem's internal offset order -- see
    DeviceOps.natural --, iterations per band (list), h, nnum)."""
    nb = ops.nb
    x, h, nnum, flags, iteration = _dist_start(ops, allreduce, threshold)
    enq = 0
    while enq < niter:
        k = min(batch, niter - enq)
        for _ in range(k):
            iteration()
        enq += k
        if int(flags[0].item()):
            break
    return x, [int(v) for v in flags[2 + nb:2 + 2 * nb].tolist()], h, nnum


def _dist_start(ops, allreduce, threshold):
    """The batched multi-rank CG drivers' common start: the global weight map and naive
    numerator, x = 0, r = p = b, the device scalars and stop flags, and the iteration
    closure over them.  Returns (x, h, nnum, flags, iteration)."""
    nb = ops.nb
    h0, _, n0 = ops.local_maps()
    h = allreduce(h0)
    nnum = allreduce(n0)
    NO = ops.n_offsets
    x, r, q = ops.zeros(NO * nb), ops.zeros(NO * nb), ops.zeros(NO * nb)
    num = ops.zeros(ops.npix * nb)
    ops.project(None, nnum, h, r)
    p = ops.copy(r)
    scal = ops.zeros(4 * nb + 1)        # rr0, rr, pq, rr_new (nb each), threshold
    ops.dot(r, r, scal[0:nb])
    allreduce(scal[0:nb])
    scal[nb:2 * nb].copy_(scal[0:nb])
    scal[3 * nb:4 * nb].copy_(scal[0:nb])
    scal[4 * nb] = float(threshold)
    flags = ops.torch.zeros(2 + 2 * nb, dtype=ops.torch.int32, device=ops.dev)
    return x, h, nnum, flags, _dist_iteration(ops, allreduce, p, num, h, q, scal, flags, x, r)


def _dist_iteration(ops, allreduce, p, num, h, q, scal, flags, x, r):
    """One multi-rank CG iteration as a no-argument callable: 4 native calls cut at the three
    all-reduces.  An operator with ``dist_parts`` (DeviceOps) runs the native solve's 4 kernels
    and all-reduces the p.q / r.r block partials (comap_destripe_dist_*_parts / _fused); any
    other (GroundOps) leaves its sums in scal, whose p.q and r.r are all-reduced."""
    nb = ops.nb
    if hasattr(ops, 'dist_parts'):
        pq_part, rr_part = ops.dist_parts()

        def parts():
            ops.dist_bin(p, num, flags)
            allreduce(num)
            ops.dist_project_parts(p, num, h, q, pq_part, flags)
            allreduce(pq_part)
            ops.dist_update_fused(scal, pq_part, x, r, p, q, rr_part, flags)
            allreduce(rr_part)
            ops.dist_direction_fused(scal, rr_part, p, r, flags)
        return parts

    def sums():
        ops.dist_bin(p, num, flags)
        allreduce(num)
        ops.dist_project(p, num, h, q, scal, flags)
        allreduce(scal[2 * nb:3 * nb])
        ops.dist_update(scal, x, r, p, q, flags)
        allreduce(scal[3 * nb:4 * nb])
        ops.dist_direction(scal, p, r, flags)
    return sums


def cg_solve_graph(ops, allreduce, threshold=1e-6, niter=100, batch=16):
    """cg_solve_batched with each batch of ``batch`` iterations -- the four kernel
    pieces AND the three all-reduces of every iteration -- captured once into a
    HIP graph (torch.cuda.graph; RCCL collectives are capturable) and replayed:
    one graph launch per batch instead of 7 host calls per iteration.  Same
    iterates, bit for bit, as cg_solve_batched (same kernels, same sums).  The
    remainder niter % batch runs eagerly.  Returns like cg_solve_batched."""
    torch = ops.torch
    nb = ops.nb
    x, h, nnum, flags, iteration = _dist_start(ops, allreduce, threshold)

    nfull = niter // batch
    graph = None
    if nfull:
        side = torch.cuda.Stream(ops.dev)
        side.wait_stream(torch.cuda.current_stream(ops.dev))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(batch):
                iteration()
    done = 0
    for _ in range(nfull):
        graph.replay()
        done += batch
        if int(flags[0].item()):
            break
    if not int(flags[0].item()):
        for _ in range(niter - done):
            iteration()
    return x, [int(v) for v in flags[2 + nb:2 + 2 * nb].tolist()], h, nnum


class _Vectors:
    """The vector helpers of cg_solve's protocol on float64 device tensors (self.torch, self.dev)."""

    def zeros(self, n):
        return self.torch.zeros(n, dtype=self.torch.float64, device=self.dev)

    def scalar(self):
        return self.zeros(1)

    def copy(self, a):
        return a.clone()

    def host_scalar(self, s):
        return float(s.item())

    def set_scalar(self, dst, src):
        dst.copy_(src)


class DeviceOps(_Vectors):
    """One rank's destriper operator on the GPU (comap_destripe_* C ABI).

    ``tod``/``weights`` are [N] (one band) or [n_bands, N] (several sidebands on
    the same ``pixels``, solved as one batched system -- comap_destripe_create_bands;
    3 bands are padded to 4 with an empty band).  ``keep`` (optional, [n_bands,
    N/L]) marks the offsets each band's data prep kept.  Per-band vectors are
    interleaved band-fastest ([N/L][nb], [npix][nb])."""

    def __init__(self, pixels, tod, weights, offset_length, npix, device=None, keep=None, okey=None):
        """okey (optional): (int32 CUDA [N/L] keys, exclusive bound) -- the offsets' internal
        processing order (comap_destripe_create_keyed); default: each offset's first on-map
        pixel."""
        import torch
        self.torch = torch
        self.dev = _device(device)
        self.ctx = N.ctx(self.dev.index)
        self.pix = self._t(pixels, torch.int32)
        tod2 = self._t2(tod, torch.float64)
        w2 = self._t2(weights, torch.float64)
        self.n_bands = int(tod2.shape[0])           # bands the caller asked for
        if w2.shape != tod2.shape:
            raise ValueError('tod and weights must have the same shape')
        if self.n_bands not in (1, 2, 3, 4):
            raise ValueError('1 to 4 bands per problem')
        self.nb = 4 if self.n_bands == 3 else self.n_bands
        n = int(tod2.shape[1])
        if self.pix.numel() != n:
            raise ValueError('pointing, tod and weights must have the same length')
        if n % offset_length:
            raise ValueError('number of samples must be a multiple of offset_length')
        # (pixel indices >= npix are caught by the set-up's count pass on the device: rc -3)
        self.L, self.npix = int(offset_length), int(npix)
        kp = None
        if keep is not None:
            kp = self._t2(keep, torch.uint8)
            if kp.shape != (self.n_bands, n // self.L):
                raise ValueError('keep must be [n_bands, n_samples // offset_length]')
        if self.nb != self.n_bands:              # pad 3 -> 4 bands with an empty band
            z = torch.zeros((1, n), dtype=torch.float64, device=self.dev)
            tod2, w2 = torch.cat([tod2, z]), torch.cat([w2, z])
            if kp is not None:
                kp = torch.cat([kp, torch.zeros((1, n // self.L), dtype=torch.uint8, device=self.dev)])
        self.tod, self.w, self.keep = tod2.contiguous(), w2.contiguous(), kp
        h = ctypes.c_void_p()
        N.bind_stream(self.ctx, self.dev)
        keys, kmax = okey if okey is not None else (None, 0)
        if keys is not None and (keys.numel() != n // self.L or keys.dtype != torch.int32):
            raise ValueError('okey must be int32 [n_samples // offset_length]')
        rc = N.lib().comap_destripe_create_keyed(self.ctx, N.dptr(self.pix), N.dptr(self.tod), N.dptr(self.w),
                                                 None if kp is None else N.dptr(kp),
                                                 None if keys is None else N.dptr(keys), int(kmax), n, self.L,
                                                 self.npix, self.nb, ctypes.byref(h))
        if rc == -3:
            raise IndexError(f'pixel index out of range for a map of {npix} pixels (valid: -{npix} .. {npix - 1})')
        N.check(rc, self.ctx, 'comap_destripe_create_bands')
        self.h = h
        self.n_offsets = int(N.lib().comap_destripe_n_offsets(h))
        self.parent = None                          # (a solve-mask view's parent: masked_view)

    def masked_view(self, mask_internal):
        """The solve-mask view of this problem (comap_destripe_mask_view) as an ops object of its
        own: the system of w' = w outside the masked pixels, 0 on them.  ``mask_internal``: uint8
        CUDA [npix] in the problem's internal pixel order, non-zero = masked.  The view shares
        ``pix``, ``tod`` and ``w`` and keeps this object alive; its native solves run the CG on
        the view and bin the final maps from this problem (comap_destripe_solve_view)."""
        torch = self.torch
        if self.parent is not None:
            raise ValueError('a solve-mask view of a view is not supported')
        m = mask_internal
        if not isinstance(m, torch.Tensor) or m.dtype != torch.uint8 or m.numel() != self.npix or not m.is_cuda:
            raise ValueError(f'solve mask must be a uint8 device tensor with {self.npix} values (one per pixel)')
        m = m.contiguous().reshape(-1)
        v = object.__new__(DeviceOps)
        v.__dict__.update({k: getattr(self, k) for k in ('torch', 'dev', 'ctx', 'pix', 'tod', 'w', 'keep', 'n_bands',
                                                          'nb', 'L', 'npix', 'n_offsets')})
        v.h, v.parent, v.mask = None, self, m
        h = ctypes.c_void_p()
        N.bind_stream(self.ctx, self.dev)
        N.check(N.lib().comap_destripe_mask_view(self.h, N.dptr(self.pix), N.dptr(self.tod), N.dptr(self.w), N.dptr(m),
                                                 ctypes.byref(h)), self.ctx, 'comap_destripe_mask_view')
        v.h = h
        return v

    def _t(self, a, dt):
        return _to_tensor(a, self.dev, dt).contiguous().reshape(-1)

    def _t2(self, a, dt):
        t = _to_tensor(a, self.dev, dt)
        return t.reshape(1, -1).contiguous() if t.dim() == 1 else t.contiguous()

    def natural(self, x):
        """Offset vector in the caller's offset order (the C side processes offsets in
        a spatially sorted internal order; every other vector here is internal)."""
        out = self.zeros(self.n_offsets * self.nb)
        self._c('comap_destripe_offsets_natural', self.h, self._v(x), self._v(out))
        return out

    def split_bands(self, v):
        """[n*nb] interleaved -> [n_bands, n] (contiguous copy, padding band dropped)."""
        return v.reshape(-1, self.nb).t()[:self.n_bands].contiguous()

    def __del__(self):
        try:
            if getattr(self, 'h', None) is not None:
                self.torch.cuda.synchronize(self.dev)
                N.lib().comap_destripe_destroy(self.h)
                self.h = None
        except Exception:  # pragma: no cover
            pass

    def nnz(self):
        a = ctypes.c_int64()
        b = ctypes.c_int64()
        N.lib().comap_destripe_nnz(self.h, ctypes.byref(a), ctypes.byref(b))
        return int(a.value), int(b.value)

    def entry_bytes(self):
        """Bytes per operator entry: 4 + NB (count form) or 4 + 8 NB."""
        return int(N.lib().comap_destripe_entry_bytes(self.h))

    def sell_entries(self):
        """Padded entries of the projection's sliced-ELLPACK rows (-1: none)."""
        return int(N.lib().comap_destripe_sell_entries(self.h))

    # ---- vector helpers
    def empty(self, n):
        """[n] float64 on the device, uninitialised (for outputs a call writes in full)."""
        return N.device_empty(n, self.torch.float64, self.dev)

    def _c(self, fn, *args):
        N.bind_stream(self.ctx, self.dev)
        N.check(getattr(N.lib(), fn)(*args), self.ctx, fn)

    # ---- operand checks: every device buffer handed to the C ABI must hold what the
    # kernels index (offset vectors [N/L * nb], maps [npix * nb], nb scalars, ...)
    def _v(self, t):
        if t.numel() < self.n_offsets * self.nb or t.dtype != self.torch.float64:
            raise ValueError(f'offset vector must be float64 with >= {self.n_offsets * self.nb} values')
        return N.dptr(t)

    def _m(self, t):
        if t.numel() < self.npix * self.nb or t.dtype != self.torch.float64:
            raise ValueError(f'map must be float64 with >= {self.npix * self.nb} values')
        return N.dptr(t)

    def _s(self, t, n=None):
        n = self.nb if n is None else n
        if t.numel() < n or t.dtype != self.torch.float64:
            raise ValueError(f'scalar buffer must be float64 with >= {n} values')
        return N.dptr(t)

    def _f(self, t):
        if t.numel() < 2 + 2 * self.nb or t.dtype != self.torch.int32:
            raise ValueError(f'flags must be int32 with >= {2 + 2 * self.nb} values')
        return N.dptr(t)

    # ---- operator pieces
    def local_maps(self):
        h, hits, nn = (self.zeros(self.npix * self.nb) for _ in range(3))
        self._c('comap_destripe_local_maps', self.h, self._m(h), self._m(hits), self._m(nn))
        return h, hits, nn

    def bin(self, x, mode, out):
        self._c('comap_destripe_bin', self.h, self._v(x), int(mode), self._m(out))

    def project(self, x, num, h, y, dot=None):
        self._c('comap_destripe_project', self.h, None if x is None else self._v(x), self._m(num), self._m(h),
                self._v(y), None if dot is None else self._s(dot))

    def dot(self, a, b, out):
        self._c('comap_destripe_dot', self.h, self._v(a), self._v(b), self._s(out))

    def cg_update(self, rr, pq, x, r, p, q, rr_new):
        self._c('comap_destripe_cg_update', self.h, self._s(rr), self._s(pq), self._v(x), self._v(r), self._v(p),
                self._v(q), self._s(rr_new))

    def cg_direction(self, rr_new, rr, p, r):
        self._c('comap_destripe_cg_direction', self.h, self._s(rr_new), self._s(rr), self._v(p), self._v(r))

    # ---- multi-rank iteration pieces (device stop flags; see cg_solve_batched): the native
    # solve's 4 launches, with the p.q / r.r block partials all-reduced between them
    def dist_bin(self, p, num, flags):
        self._c('comap_destripe_dist_bin', self.h, self._v(p), self._m(num), self._f(flags))

    def dist_parts(self):
        """Zeroed [nb * comap_destripe_dist_parts()] partial buffers for p.q and r.r."""
        n = int(N.lib().comap_destripe_dist_parts()) * self.nb
        return self.zeros(n), self.zeros(n)

    def _pp(self, t):
        n = int(N.lib().comap_destripe_dist_parts()) * self.nb
        if t.numel() < n or t.dtype != self.torch.float64:
            raise ValueError(f'partial buffer must be float64 with >= {n} values')
        return N.dptr(t)

    def dist_project_parts(self, p, num, h, q, pq_part, flags):
        self._c('comap_destripe_dist_project_parts', self.h, self._v(p), self._m(num), self._m(h), self._v(q),
                self._pp(pq_part), self._f(flags))

    def dist_update_fused(self, scal, pq_part, x, r, p, q, rr_part, flags):
        self._c('comap_destripe_dist_update_fused', self.h, self._s(scal, 4 * self.nb + 1), self._pp(pq_part),
                self._v(x), self._v(r), self._v(p), self._v(q), self._pp(rr_part), self._f(flags))

    def dist_direction_fused(self, scal, rr_part, p, r, flags):
        self._c('comap_destripe_dist_direction_fused', self.h, self._s(scal, 4 * self.nb + 1), self._pp(rr_part),
                self._v(p), self._v(r), self._f(flags))

    def div_map(self, num, h, out):
        self._c('comap_destripe_div_map', self.h, self._m(num), self._m(h), self._m(out))

    # ---- split maps (per-label maps of a solved problem, comap_destripe_split_maps)
    def split_maps(self, x, labels, n_labels):
        """The raw sums (num, naive_num, weight, hits), each [n_labels * npix * nb] (label, pixel,
        band fastest), of this rank's samples per label: ``labels`` int32 CUDA [N/L] in
        [-1, n_labels), ``x`` [N/L * nb] in the CALLER's offset order (``natural``; the native
        solve's x).  IndexError for a pixel id out of range, ValueError for a label."""
        torch = self.torch
        G = int(n_labels)
        if labels.numel() != self.n_offsets or labels.dtype != torch.int32:
            raise ValueError(f'split labels must be int32 with {self.n_offsets} values (one per offset)')
        if G < 1 or G * self.npix >= 2 ** 31:
            raise ValueError(f'n_labels * npix must lie in [1, 2^31), not {G} * {self.npix}')
        out = [self.empty(G * self.npix * self.nb) for _ in range(4)]        # written in full
        N.bind_stream(self.ctx, self.dev)
        rc = N.lib().comap_destripe_split_maps(self.ctx, N.dptr(self.pix), N.dptr(self.tod), N.dptr(self.w),
                                               None if self.keep is None else N.dptr(self.keep), self._v(x),
                                               N.dptr(labels), G, self.pix.numel(), self.L, self.npix, self.nb,
                                               *(N.dptr(v) for v in out))
        self._pass_rc(rc, 'comap_destripe_split_maps', 'split', G)
        return tuple(out)

    def _pass_rc(self, rc, fn, what, G):
        """The return code of a post-solve pass (split maps, residuals): -3 is a pixel id out of
        range (IndexError), -4 a label (ValueError)."""
        if rc == -3:
            raise IndexError(f'pixel index out of range for a map of {self.npix} pixels '
                             f'(valid: -{self.npix} .. {self.npix - 1})')
        if rc == -4:
            raise ValueError(f'{what} label out of range (valid: -1 .. {G - 1})')
        N.check(rc, self.ctx, fn)

    def split_div(self, num, nnum, weight):
        """(map, naive) = (num, naive_num) / weight where weight != 0, else the numerator."""
        n = num.numel()
        m, nv = self.empty(n), self.empty(n)
        self._c('comap_destripe_split_div', self.ctx, N.dptr(num), N.dptr(nnum), N.dptr(weight), n, N.dptr(m),
                N.dptr(nv))
        return m, nv

    # ---- residual chi-squared (comap_destripe_residuals)
    def residuals(self, x, m, group=None, n_groups=0):
        """(off_sum, off_cnt, grp_sum, grp_cnt) of this rank's samples against the solved offsets
        ``x`` ([N/L * nb], the CALLER's offset order: ``natural``, the native solve's x) and the
        map ``m`` ([npix * nb] in the problem's internal pixel layout, i.e. before the
        destriper's expansion and un-tiling): per offset and band the sum of (w r) r, r = (tod -
        x) - m[pix], over the counted samples (pix >= 0, w > 0, the band kept the offset) in the
        lane-tree order (``lane_tree_sum``) and their number, [N/L * nb] float64 / int32; per
        group the lane-tree sum of its offsets' sums in increasing offset and the sum of their
        counts, [n_groups * nb] float64 / int64 (None without ``group``: int32 CUDA [N/L] in
        [-1, n_groups), -1 = in no group).  A non-finite tod makes its sums NaN.  IndexError for a
        pixel id out of range, ValueError for a label."""
        torch = self.torch
        G = int(n_groups)
        if group is not None:
            if group.numel() != self.n_offsets or group.dtype != torch.int32:
                raise ValueError(f'residual groups must be int32 with {self.n_offsets} values (one per offset)')
            if G < 1:
                raise ValueError(f'n_groups must be >= 1 with group labels, not {G}')
        elif G != 0:
            raise ValueError('n_groups without group labels')
        n = self.n_offsets * self.nb
        off_sum, off_cnt = self.empty(n), N.device_empty(n, torch.int32, self.dev)     # written in full
        grp_sum = grp_cnt = None
        if group is not None:
            grp_sum, grp_cnt = self.empty(G * self.nb), N.device_empty(G * self.nb, torch.int64, self.dev)
        N.bind_stream(self.ctx, self.dev)
        rc = N.lib().comap_destripe_residuals(self.ctx, N.dptr(self.pix), N.dptr(self.tod), N.dptr(self.w),
                                              None if self.keep is None else N.dptr(self.keep), self._v(x),
                                              self._m(m), None if group is None else N.dptr(group), G,
                                              self.pix.numel(), self.L, self.npix, self.nb, N.dptr(off_sum),
                                              N.dptr(off_cnt), None if group is None else N.dptr(grp_sum),
                                              None if group is None else N.dptr(grp_cnt))
        self._pass_rc(rc, 'comap_destripe_residuals', 'residual group', G)
        return off_sum, off_cnt, grp_sum, grp_cnt

    # ---- single-rank native solve (no Python per iteration)
    def solve_native(self, threshold, niter):
        """x [N/L * nb], iterations per band (list), maps {k: [npix * nb]} (interleaved)."""
        nb = self.nb
        x = self.empty(self.n_offsets * nb)                  # the solve writes x and every map in full
        maps = {k: self.empty(self.npix * nb) for k in ('map', 'naive', 'weight', 'hits')}
        it = (ctypes.c_int32 * nb)()
        # (a solve-mask view: its CG, then the maps from its parent)
        self._c('comap_destripe_solve' if self.parent is None else 'comap_destripe_solve_view', self.h,
                float(threshold), int(niter), N.dptr(x), N.dptr(maps['map']),
                N.dptr(maps['naive']), N.dptr(maps['weight']), N.dptr(maps['hits']),
                ctypes.cast(it, ctypes.POINTER(ctypes.c_int32)))
        return x, [int(v) for v in it][:self.n_bands], maps

    def solve_native_host(self, threshold, niter, unmap=None):
        """solve_native with the maps delivered to the host: {k: NumPy [n_bands, npix]}.
        naive / weight / hits do not depend on the offsets, so they are formed and
        copied to pinned host memory on a copy stream while the CG runs; only the
        destriped map is copied after the solve (bench.py's chain: 0.73 ms of map copy
        -> ~0.2 ms)."""
        torch = self.torch
        nb, npix, nbo = self.nb, self.npix, self.n_bands
        cur = torch.cuda.current_stream(self.dev)
        m = N.device_empty((4, npix * nb), torch.float64, self.dev)              # map, naive, weight, hits
        nn = self.empty(npix * nb)                                              # local_maps copies it in full
        full = self.h if self.parent is None else self.parent.h                 # (a view's maps are its parent's)
        self._c('comap_destripe_local_maps', full, N.dptr(m[2]), N.dptr(m[3]), N.dptr(nn))
        self._c('comap_destripe_div_map', full, N.dptr(nn), None, N.dptr(m[1]))
        bands = m.view(4, npix, nb).permute(0, 2, 1)[:, :nbo]                    # [4, n_bands, npix] view
        # unmap: the caller's pixel order from the problem's internal (tiled) one
        static = bands[1:].contiguous() if unmap is None else bands[1:].index_select(2, unmap)
        # page-locked result block from the library's host cache (torch's pinned
        # allocator paid a fresh ~2.5 ms hipHostMalloc on every other solve, r03s7)
        host_np = N.host_empty((4, nbo, npix if unmap is None else int(unmap.numel())))
        host = torch.from_numpy(host_np)
        ready = torch.cuda.Event()
        ready.record(cur)
        cs = copy_stream(self.dev)
        cs.wait_event(ready)
        with torch.cuda.stream(cs):
            host[1:].copy_(static, non_blocking=True)
        static.record_stream(cs)
        x = self.empty(self.n_offsets * nb)                                     # written in full by the solve
        it = (ctypes.c_int32 * nb)()
        self._c('comap_destripe_solve' if self.parent is None else 'comap_destripe_solve_view', self.h,
                float(threshold), int(niter), N.dptr(x), N.dptr(m[0]), None, None,
                None, ctypes.cast(it, ctypes.POINTER(ctypes.c_int32)))
        host[0].copy_(bands[0] if unmap is None else bands[0].index_select(1, unmap), non_blocking=True)
        cur.synchronize()
        cs.synchronize()
        maps = {k: host_np[i] for i, k in enumerate(('map', 'naive', 'weight', 'hits'))}
        return x, [int(v) for v in it][:nbo], maps


def ground_groups(feedid, obsids, offset_length):
    """Ground-template group of every offset: (gid int32 [N/L], unique_obsids, unique_feeds).

    Group k = i * n_feeds + j for observation i of np.unique(obsids) and feed j of
    np.unique(feedid), the reference's order (op_Ax_with_ground, Destriper.py:279-287); a
    combination without samples is simply a group no offset belongs to.  The device operator
    works on whole offsets, so every offset must lie in one group (read_comap_data keeps
    floor(n / L) * L samples per feed and scan, which guarantees it): ValueError otherwise,
    and when the lengths disagree or are no multiple of offset_length."""
    feedid, obsids = np.asarray(feedid).reshape(-1), np.asarray(obsids).reshape(-1)
    L = int(offset_length)
    if feedid.size != obsids.size:
        raise ValueError(f'feedid ({feedid.size}) and obsids ({obsids.size}) must have the same length')
    if L < 1 or feedid.size % L:
        raise ValueError(f'{feedid.size} samples are not a multiple of offset_length {L}')
    uobs, iobs = np.unique(obsids, return_inverse=True)
    ufeed, ifeed = np.unique(feedid, return_inverse=True)
    gid = (iobs.reshape(-1) * ufeed.size + ifeed.reshape(-1)).reshape(-1, L)
    if gid.size and np.any(gid != gid[:, :1]):
        bad = int(np.nonzero(np.any(gid != gid[:, :1], axis=1))[0][0])
        raise ValueError(f'offset {bad} straddles two (observation, feed) groups: the ground template needs '
                         'every offset inside one group')
    return gid[:, 0].astype(np.int32), uobs, ufeed


def merge_ground_tables(tables):
    """One ground-fit table from every rank's: the table a single rank holding all samples
    would report.  ``tables``: per rank {'obsids' [n_obs], 'feeds' [n_feeds], 'slope', 'level',
    'wrapped', 'held' [n_obs, n_feeds]} over the rank's own np.unique grids, 'held' marking the
    (observation, feed) pairs the rank has samples of.  The result spans the union of
    observations x the union of feeds, both sorted; a pair no rank holds is 0 / not wrapped.
    ValueError when two ranks hold the same pair: its template must live on one rank, or it
    would be fitted twice."""
    obs = [np.asarray(t['obsids']).reshape(-1) for t in tables]
    feeds = [np.asarray(t['feeds']).reshape(-1) for t in tables]
    uobs = np.unique(np.concatenate(obs)) if obs else np.zeros(0)
    ufeed = np.unique(np.concatenate(feeds)) if feeds else np.zeros(0)
    shape = (uobs.size, ufeed.size)
    out = {'obsids': uobs, 'feeds': ufeed, 'slope': np.zeros(shape), 'level': np.zeros(shape),
           'wrapped': np.zeros(shape, bool)}
    owner = np.full(shape, -1, np.int64)
    for rank, t in enumerate(tables):
        held = np.asarray(t['held'], bool).reshape(obs[rank].size, feeds[rank].size)
        io, jf = np.nonzero(held)
        gi, gj = np.searchsorted(uobs, obs[rank])[io], np.searchsorted(ufeed, feeds[rank])[jf]
        twice = owner[gi, gj] >= 0
        if np.any(twice):
            k = int(np.nonzero(twice)[0][0])
            raise ValueError(f'observation {uobs[gi[k]]}, feed {ufeed[gj[k]]} has samples on ranks '
                             f'{int(owner[gi[k], gj[k]])} and {rank}: the ground template of one (observation, feed) '
                             'must live on one rank')
        owner[gi, gj] = rank
        for key in ('slope', 'level', 'wrapped'):
            if t.get(key) is not None:
                out[key][gi, gj] = np.asarray(t[key]).reshape(held.shape)[io, jf]
    return out


def _agree(d, what, error, payload=None):
    """Every rank's status (``error``: its exception or None) and ``payload`` exchanged in one
    all_gather_object, so that all ranks raise or none does (a rank that raised alone would leave
    its peers waiting in the next collective): the failing rank raises its own exception, the
    others ValueError.  Returns every rank's payload in rank order."""
    everyone = [None] * d.get_world_size()
    d.all_gather_object(everyone, (None if error is None else (type(error).__name__, str(error)), payload))
    for rank, (err, _) in enumerate(everyone):
        if err is not None:
            if rank == d.get_rank():
                raise error
            raise ValueError(f'{what} failed on rank {rank}: {err[0]}: {err[1]}')
    return [v for _, v in everyone]


def _on_every_rank(what, step, catch=ValueError, payload=None):
    """(step(), every rank's payload(step()) in rank order) -- the local ``step`` of ``what``
    ('split maps', 'residuals', ...) under the ranks' rule: on one rank its exception propagates
    (and the payloads are None); across ranks an exception of the types ``catch`` is held back,
    exchanged (_agree: one all_gather_object, before the collectives the step protects) and raised
    on every rank or on none."""
    d = _dist()
    if d is None or d.get_world_size() == 1:
        return step(), None
    error = result = mine = None
    try:
        result = step()
        mine = None if payload is None else payload(result)
    except catch as e:
        error = e
    return result, _agree(d, what, error, mine)


SPLIT_KEYS = ('map', 'naive', 'weight', 'hits')


def residual_group_labels(feedid, obsids, offset_length):
    """The residual table's (observation, feed) group of every offset: (gid int32 [N/L],
    unique_obsids, unique_feeds), ``ground_groups``' labels (group = i n_feeds + j; an offset
    that straddles two groups raises ValueError) -- across ranks over the union of all ranks'
    observations and feeds, taken as ``split_specs`` takes its labels, so that group g means the
    same on every rank; a rank's ValueError is raised on every rank."""
    mine, every = _on_every_rank('residuals', lambda: ground_groups(feedid, obsids, offset_length),
                                 payload=lambda m: (m[1], m[2]))
    if every is None:
        return mine
    gid, uobs, ufeed = mine
    aobs = np.unique(np.concatenate([np.asarray(v[0]).reshape(-1) for v in every]))
    afeed = np.unique(np.concatenate([np.asarray(v[1]).reshape(-1) for v in every]))
    i, j = np.searchsorted(aobs, uobs)[gid // ufeed.size], np.searchsorted(afeed, ufeed)[gid % ufeed.size]
    return (i * afeed.size + j).astype(np.int32), aobs, afeed


def _offset_values(by, feedid, obsids, offset_length):
    """The feed (by='feed') or observation (by='obsid') of every offset, [N/L]; ValueError when
    it changes inside an offset or the samples are no whole offsets."""
    if by not in ('feed', 'obsid'):
        raise ValueError(f"split must be 'feed' or 'obsid', not {by!r}")
    v = np.asarray(feedid if by == 'feed' else obsids).reshape(-1)
    L = int(offset_length)
    if L < 1 or v.size % L:
        raise ValueError(f'{v.size} samples are not a multiple of offset_length {L}')
    v = v.reshape(-1, L)
    if v.size and np.any(v != v[:, :1]):
        bad = int(np.nonzero(np.any(v != v[:, :1], axis=1))[0][0])
        raise ValueError(f'offset {bad} straddles two {by}s: a split map needs every offset inside one')
    return v[:, 0] if v.size else v.reshape(-1)


def _labels_in(by, v, values):
    """(labels int32, names) of the per-offset values ``v`` in the label set ``values``."""
    members = np.unique(np.asarray(values).reshape(-1))
    lab = np.searchsorted(members, v)
    inside = lab < members.size
    inside[inside] = members[lab[inside]] == v[inside]
    lab = np.where(inside, lab, -1).astype(np.int32)
    return lab, [f'Feed{int(m):02d}' if by == 'feed' else f'Obs{int(m)}' for m in members]


def split_labels(by, feedid, obsids, offset_length, values=None):
    """Split-map label of every offset: (labels int32 [N/L], names).

    by='feed': label j for feed np.unique(feedid)[j], named f'Feed{feed:02d}' (the reference's
    spelling, Destriper.py:487-501); by='obsid': label i for observation np.unique(obsids)[i],
    named f'Obs{int(obsid)}'.  ``values`` fixes the label set instead (sorted and made unique;
    ranks pass the union over ranks, so that label g means the same on every rank): a member
    without samples is a label that owns no offset, and a sample whose feed / observation is not
    a member gets label -1 (in no split).  The device pass works on whole offsets, so a feed or
    observation that changes inside an offset raises ValueError, as do per-sample arrays whose
    length is no multiple of offset_length (as ``ground_groups``)."""
    v = _offset_values(by, feedid, obsids, offset_length)
    return _labels_in(by, v, v if values is None else values)


def split_specs(split, feedid, obsids, offset_length):
    """run_destriper's ``split`` ('feed', 'obsid' or a list of these) as [(labels, names)] per
    requested split, the label values being the union over ranks; a rank's ValueError (a label
    changing inside an offset, ...) is raised on every rank.  None / empty: None."""
    if split is None or (not isinstance(split, str) and len(split) == 0):
        return None
    kinds = [split] if isinstance(split, str) else list(split)
    if feedid is None or obsids is None:
        raise ValueError('split maps need feedid and obsids')
    def local():
        per_offset = [_offset_values(by, feedid, obsids, offset_length) for by in kinds]
        return per_offset, [np.unique(v) for v in per_offset]

    (per_offset, values), every = _on_every_rank('split maps', local, payload=lambda r: r[1])
    if every is not None:
        values = [np.concatenate([r[i] for r in every]) for i in range(len(kinds))]
    return [_labels_in(by, v, vals) for by, v, vals in zip(kinds, per_offset, values)]


class GroundOps(_Vectors):
    """The destriper operator with a ground (azimuth) template per (observation, feed):
    the reference's op_Ax_with_ground (Destriper.py:265-336) as the operator object that
    ``cg_solve`` and ``cg_solve_batched`` drive (comap_destripe_ground_* around a DeviceOps' own
    calls).

    Vectors hold [x (N/L offsets, internal order) | s (K slopes) | c (K levels)], groups in
    ``ground_groups`` order.  The azimuth enters centred and scaled per group, a = (az -
    mu_k) / sigma_k (0 for a constant azimuth) -- see ``fit`` for the reference's units.  The
    offsets' part of every vector runs through the plain problem's kernels, the 2K-value
    tails through comap_destripe_ground_tail_* (no host synchronisation)."""

    def __init__(self, ops, az, gid, n_groups):
        torch = ops.torch
        if ops.nb != 1:
            raise NotImplementedError('the ground template solves one band (batched bands are not supported)')
        self.ops, self.torch, self.dev, self.ctx, self.nb = ops, torch, ops.dev, ops.ctx, 1
        self.K, self.NO, self.npix = int(n_groups), ops.n_offsets, ops.npix
        self.n_offsets = self.NO + 2 * self.K
        az = ops._t(az, torch.float64)
        gid = ops._t(gid, torch.int32)
        if az.numel() != ops.pix.numel():
            raise ValueError('az must have one value per sample')
        if gid.numel() != self.NO:
            raise ValueError('one ground group id per offset')
        g = ctypes.c_void_p()
        N.bind_stream(self.ctx, self.dev)
        rc = N.lib().comap_destripe_ground_create(ops.h, N.dptr(ops.pix), N.dptr(az), N.dptr(ops.tod), N.dptr(ops.w),
                                                  N.dptr(gid), self.K, ctypes.byref(g))
        if rc == -3:
            raise IndexError(f'ground template: {N.lib().comap_last_error(self.ctx).decode()}')
        N.check(rc, self.ctx, 'comap_destripe_ground_create')
        self.g = g
        self.xp = ops.zeros(self.NO)                 # x' = x + c[g(o)], the level folded into the offsets
        self._folded = None                          # (vector, its version) xp was folded from by bin()
        self.mu, self.sigma = ops.zeros(self.K), ops.zeros(self.K)
        self._c('comap_destripe_ground_stats', self.g, N.dptr(self.mu), N.dptr(self.sigma))
        # groups crossing azimuth 0 / 360 (raw span > 180 deg): their az < 180 entered as az + 360
        self.wrapped = torch.zeros(self.K, dtype=torch.int32, device=self.dev)
        self._c('comap_destripe_ground_wrapped', self.g, N.dptr(self.wrapped))

    def __del__(self):
        try:
            if getattr(self, 'g', None) is not None:
                self.torch.cuda.synchronize(self.dev)
                N.lib().comap_destripe_ground_destroy(self.g)
                self.g = None
        except Exception:  # pragma: no cover
            pass

    def _c(self, fn, *args):
        self.ops._c(fn, *args)

    def nnz(self):
        """(group, pixel) entries: (group-major incl. off-map reads, pixel-major binned only)."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        N.lib().comap_destripe_ground_nnz(self.g, ctypes.byref(a), ctypes.byref(b))
        return int(a.value), int(b.value)

    def local_maps(self):
        return self.ops.local_maps()

    def _u(self, t):
        if t.numel() != self.n_offsets or t.dtype != self.torch.float64 or not t.is_contiguous():
            raise ValueError(f'ground vector must be contiguous float64 with {self.n_offsets} values')
        return t

    def split(self, u):
        """(x [N/L] internal order, s [K], c [K]) views of a vector."""
        u = self._u(u)
        return u[:self.NO], u[self.NO:self.NO + self.K], u[self.NO + self.K:]

    def _fold(self, u, reuse=False):
        """x' for vector u into self.xp; returns u's slopes.  reuse: project(u) right after
        bin(u), as cg_solve calls them, keeps bin's x' (every call here that writes a vector
        forgets it: the native kernels write behind torch's version counter)."""
        x, s, c = self.split(u)
        f = self._folded
        if not (reuse and f is not None and f[0] is u and f[1] == u._version):
            self._c('comap_destripe_ground_fold', self.g, N.dptr(x), N.dptr(c), N.dptr(self.xp))
        self._folded = (u, u._version)
        return s

    def _tail(self, t):
        return N.dptr(self._u(t)[self.NO:])

    # ---- operator pieces
    def bin(self, u, mode, out):
        """mode 0: num = [W F | W G] u; mode 1: the destriped map's numerator, naive - that."""
        s = self._fold(u)
        self.ops.bin(self.xp, mode, out)
        self._c('comap_destripe_ground_bin', self.g, N.dptr(s if mode == 0 else -s), self.ops._m(out))

    def project(self, u, num, h, y, dot=None):
        y = self._u(y)
        if u is None:                                 # b: the offsets' rows, then the tail from them
            self._folded = None
            self.ops.project(None, num, h, y)
            self._c('comap_destripe_ground_rhs', self.g, self.ops._m(num), self.ops._m(h), N.dptr(y), self._tail(y))
            return
        s = self._fold(u, reuse=True)
        self._folded = None
        self.ops.project(self.xp, num, h, y)
        self._c('comap_destripe_ground_project', self.g, N.dptr(self.xp), N.dptr(s), self.ops._m(num), self.ops._m(h),
                N.dptr(y), self._tail(y))
        if dot is not None:
            self.dot(u, y, dot)

    def dot(self, a, b, out):
        self.ops.dot(self._u(a), self._u(b), out)
        self._c('comap_destripe_ground_tail_dot', self.g, self._tail(a), self._tail(b), self.ops._s(out))

    def cg_update(self, rr, pq, x, r, p, q, rr_new):
        self._folded = None
        self.ops.cg_update(rr, pq, self._u(x), self._u(r), self._u(p), self._u(q), rr_new)
        self._c('comap_destripe_ground_tail_update', self.g, self.ops._s(rr), self.ops._s(pq), self._tail(x),
                self._tail(r), self._tail(p), self._tail(q), self.ops._s(rr_new))

    def cg_direction(self, rr_new, rr, p, r):
        self._folded = None
        self.ops.cg_direction(rr_new, rr, self._u(p), self._u(r))
        self._c('comap_destripe_ground_tail_direction', self.g, self.ops._s(rr_new), self.ops._s(rr), self._tail(p),
                self._tail(r))

    # ---- multi-rank iteration pieces (device stop flags; see cg_solve_batched)
    def dist_bin(self, p, num, flags):
        self._folded = None
        self._c('comap_destripe_ground_dist_bin', self.g, N.dptr(self._u(p)), self.ops._m(num), self.ops._f(flags))

    def dist_project(self, p, num, h, q, scal, flags):
        self._c('comap_destripe_ground_dist_project', self.g, N.dptr(self._u(p)), self.ops._m(num), self.ops._m(h),
                N.dptr(self._u(q)), self.ops._s(scal, 5), self.ops._f(flags))

    def dist_update(self, scal, x, r, p, q, flags):
        self._c('comap_destripe_ground_dist_update', self.g, self.ops._s(scal, 5), N.dptr(self._u(x)),
                N.dptr(self._u(r)), N.dptr(self._u(p)), N.dptr(self._u(q)), self.ops._f(flags))

    def dist_direction(self, scal, p, r, flags):
        self._c('comap_destripe_ground_dist_direction', self.g, self.ops._s(scal, 5), N.dptr(self._u(p)),
                N.dptr(self._u(r)), self.ops._f(flags))

    # ---- single-rank native solve (no Python per iteration)
    def solve_native(self, threshold, niter):
        """comap_destripe_ground_solve: (u [N/L + 2K] = x internal order | s | c, iterations,
        maps {k: [npix]}): ``cg_solve`` on this operator and _solve_ground's maps, run on the
        device as replayed graph batches with a device stop flag."""
        self._folded = None
        u = self.ops.empty(self.n_offsets)                    # the solve writes u and every map in full
        maps = {k: self.ops.empty(self.npix) for k in ('map', 'naive', 'weight', 'hits')}
        it = ctypes.c_int32()
        self._c('comap_destripe_ground_solve', self.g, float(threshold), int(niter), N.dptr(u), N.dptr(maps['map']),
                N.dptr(maps['naive']), N.dptr(maps['weight']), N.dptr(maps['hits']), ctypes.byref(it))
        return u, int(it.value), maps

    # ---- results
    def fit(self, u):
        """(slope [K], level [K]) in the reference's units (per degree of raw azimuth):
        slope = s / sigma, level = c - s mu / sigma (slope 0 where sigma == 0).  The level is
        defined only up to the offsets' null space: a constant moved between c_k and the
        group's offsets changes no residual, and CG from 0 returns the minimum-norm split.
        A group that crosses azimuth 0 / 360 (``self.wrapped``) was fitted on its unwrapped
        series (az + 360 where az < 180): its mu may exceed 360 and its level is relative to
        azimuth on [180, 540)."""
        _, s, c = self.split(u)
        torch = self.torch
        slope = torch.where(self.sigma > 0, s / torch.where(self.sigma > 0, self.sigma, torch.ones_like(self.sigma)),
                            torch.zeros_like(s))
        return slope, c - slope * self.mu


class PriorOps(_Vectors):
    """The destriper operator with a noise prior on the offsets, A + T (MADAM's F^T W Z F +
    C_a^-1), as the operator object ``cg_solve`` drives: comap_destripe_prior_* around a one-band
    DeviceOps' own calls.  ``gid`` holds one int32 group id per offset in the CALLER's (time)
    order, in [-1, G) with -1 = no prior, every group one contiguous run of offsets; ``stencil``
    is float64 [G, K + 1], 1 <= K <= 64 (``prior_apply_reference`` states T).  The right-hand side
    has no prior term.  Vectors are the DeviceOps' (internal offset order)."""

    def __init__(self, ops, gid, stencil):
        torch = ops.torch
        if ops.nb != 1:
            raise NotImplementedError('the noise prior solves one band (batched bands are not supported)')
        self.ops, self.torch, self.dev, self.ctx, self.nb = ops, torch, ops.dev, ops.ctx, 1
        self.n_offsets, self.npix = ops.n_offsets, ops.npix
        st = _to_tensor(stencil, ops.dev, torch.float64).contiguous()
        if st.dim() != 2 or not 1 <= st.shape[1] - 1 <= 64 or st.shape[0] < 1:
            raise ValueError('noise prior: stencil must be [n_groups >= 1, K + 1] with 1 <= K <= 64')
        gid = ops._t(gid, torch.int32)
        if gid.numel() != self.n_offsets:
            raise ValueError(f'noise prior: one group id per offset ({self.n_offsets}), not {gid.numel()}')
        self.gid, self.stencil, self.G, self.K = gid, st, int(st.shape[0]), int(st.shape[1]) - 1
        h = ctypes.c_void_p()
        N.bind_stream(self.ctx, self.dev)
        rc = N.lib().comap_destripe_prior_create(ops.h, N.dptr(gid), self.G, N.dptr(st), self.K, ctypes.byref(h))
        if rc == -3:
            raise ValueError(N.lib().comap_last_error(self.ctx).decode())
        N.check(rc, self.ctx, 'comap_destripe_prior_create')
        self.pr = h

    def __del__(self):
        try:
            if getattr(self, 'pr', None) is not None:
                self.torch.cuda.synchronize(self.dev)
                N.lib().comap_destripe_prior_destroy(self.pr)
                self.pr = None
        except Exception:  # pragma: no cover
            pass

    def _c(self, fn, *args):
        self.ops._c(fn, *args)

    def natural(self, x):
        return self.ops.natural(x)

    def local_maps(self):
        return self.ops.local_maps()

    def prior_apply(self, v, out, accumulate=0):
        """out = T v (accumulate: out += T v); v, out [N/L] in the internal offset order."""
        self._c('comap_destripe_prior_apply', self.pr, self.ops._v(v), self.ops._v(out), int(accumulate))

    # ---- operator pieces
    def bin(self, x, mode, out):
        self.ops.bin(x, mode, out)

    def project(self, u, num, h, y, dot=None):
        if u is None:                                 # b has no prior term
            self.ops.project(None, num, h, y)
            return
        # u . (A u) by the base projection's own fused dot, then u . (T u) added to it: with a zero
        # prior every bit of the plain solve stays in place (a dot of the finished vector through
        # ops.dot would sum in another order)
        self.ops.project(u, num, h, y, dot)
        if dot is None:
            self.prior_apply(u, y, accumulate=1)
        else:
            self._c('comap_destripe_prior_apply_dot', self.pr, self.ops._v(u), self.ops._v(y), 1, self.ops._s(dot))

    def dot(self, a, b, out):
        self.ops.dot(a, b, out)

    def cg_update(self, rr, pq, x, r, p, q, rr_new):
        self.ops.cg_update(rr, pq, x, r, p, q, rr_new)

    def cg_direction(self, rr_new, rr, p, r):
        self.ops.cg_direction(rr_new, rr, p, r)

    # ---- single-rank native solve (no Python per iteration)
    def solve_native(self, threshold, niter):
        """comap_destripe_prior_solve: (x [N/L] in the CALLER's offset order, [iterations], maps
        {k: [npix]}), as DeviceOps.solve_native returns them."""
        ops = self.ops
        x = ops.empty(self.n_offsets)                         # the solve writes x and every map in full
        maps = {k: ops.empty(self.npix) for k in ('map', 'naive', 'weight', 'hits')}
        it = ctypes.c_int32()
        self._c('comap_destripe_prior_solve', self.pr, float(threshold), int(niter), N.dptr(x), N.dptr(maps['map']),
                N.dptr(maps['naive']), N.dptr(maps['weight']), N.dptr(maps['hits']), ctypes.byref(it))
        return x, [int(it.value)], maps


def prior_tile():
    """The caller-order offsets one workgroup of the prior kernel takes per sweep."""
    return int(N.lib().comap_destripe_prior_tile())


def _prior_check(prior, ground, multi):
    """The combinations a noise prior does not support, raised before any device call."""
    if prior is None:
        return
    if ground is not None and ground is not False:
        raise NotImplementedError('the noise prior with the ground template is not supported')
    if multi:
        raise NotImplementedError('the noise prior solves one band: pass a 1-D tod (batched bands are not supported)')
    if isinstance(prior, dict):
        if prior.get('feedid') is None or prior.get('obsids') is None:
            raise ValueError("a noise-prior model needs 'feedid' and 'obsids' per sample")
        if 'table' not in prior and ('fknee' not in prior or 'alpha' not in prior):
            raise ValueError("a noise-prior model needs 'fknee' and 'alpha', or a 'table' of them")
    elif not (isinstance(prior, (tuple, list)) and len(prior) == 2):
        raise ValueError('prior must be (gid, stencil) or a noise-model dict')


def _mask_check(solve_mask, ground, residual_cut, healpix=False):
    """The combinations a solve mask does not support, raised before any device call."""
    if solve_mask is None:
        return
    if ground is not None and ground is not False:
        raise NotImplementedError('a solve mask with the ground template is not supported')
    if residual_cut is not None:
        raise NotImplementedError('a solve mask with residual_cut is not supported: the cut rebuilds the problem')
    if healpix:
        raise NotImplementedError('a solve mask on a HEALPix map is not supported')


def solve_mask_flags(mask, npix, map_shape=None):
    """The caller's solve mask as host uint8 [npix] (non-zero / True = masked): bool, integer or
    float values, [npix] or, with ``map_shape`` (ny, nx), [ny, nx].  ValueError for another
    length or dimension and for a non-finite value."""
    m = mask.cpu().numpy() if hasattr(mask, 'cpu') else np.asarray(mask)
    if m.dtype.kind not in 'biuf':
        raise ValueError(f'solve mask must hold bool, integer or float flags, not {m.dtype}')
    if m.dtype.kind == 'f' and not np.isfinite(m).all():
        raise ValueError('solve mask holds a non-finite value')
    if m.ndim == 2:
        if map_shape is None or tuple(int(v) for v in map_shape) != m.shape:
            raise ValueError(f'a 2-D solve mask needs map_shape = its shape {m.shape}, not {map_shape}')
    elif m.ndim != 1:
        raise ValueError(f'solve mask must be [npix] or [ny, nx], not {m.ndim}-dimensional')
    if m.size != int(npix):
        raise ValueError(f'solve mask must hold one flag per map pixel ({int(npix)}), not {m.size}')
    return (m.reshape(-1) != 0).astype(np.uint8)


def mask_from_map(m, weight, nsigma, grow=1):
    """A solve mask from a first-pass map (host NumPy): pixel p of the 2-D map ``m`` is flagged when
    weight_p > 0 and |m_p - median(m[weight > 0])| sqrt(weight_p) > nsigma; the flagged set is then
    dilated ``grow`` times with the 3 x 3 cross (a pixel's four edge neighbours, no wrap at the map's
    border).  Returns bool [ny, nx]."""
    m, weight = np.asarray(m, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    if m.ndim != 2 or weight.shape != m.shape:
        raise ValueError('mask_from_map takes a 2-D map and a weight map of the same shape')
    nsigma, grow = float(nsigma), int(grow)
    if not (np.isfinite(nsigma) and nsigma > 0) or grow < 0:
        raise ValueError(f'mask_from_map: nsigma must be positive and grow >= 0, not {nsigma}, {grow}')
    hit = weight > 0
    out = np.zeros(m.shape, bool)
    if not hit.any():
        return out
    med = np.median(m[hit])
    with np.errstate(invalid='ignore'):
        out[hit] = np.abs(m[hit] - med) * np.sqrt(weight[hit]) > nsigma
    for _ in range(grow):
        g = out.copy()
        g[1:] |= out[:-1]
        g[:-1] |= out[1:]
        g[:, 1:] |= out[:, :-1]
        g[:, :-1] |= out[:, 1:]
        out = g
    return out


def _snr_spec(solve_mask):
    """(nsigma, grow) when ``solve_mask`` is the two-pass form ('snr', nsigma[, grow]), else None."""
    if isinstance(solve_mask, (tuple, list)) and len(solve_mask) in (2, 3) and isinstance(solve_mask[0], str):
        if solve_mask[0] != 'snr':
            raise ValueError(f"solve_mask: the two-pass form is ('snr', nsigma[, grow]), not {solve_mask!r}")
        nsigma = float(solve_mask[1])
        grow = solve_mask[2] if len(solve_mask) == 3 else 1
        if not (np.isfinite(nsigma) and nsigma > 0):
            raise ValueError(f'solve_mask snr: nsigma must be a positive number, not {solve_mask[1]!r}')
        if float(grow) != int(grow) or int(grow) < 0:
            raise ValueError(f'solve_mask snr: grow must be a whole number >= 0, not {grow!r}')
        return nsigma, int(grow)
    return None


def prior_from_model(ops, model, offset_length):
    """(gid int32 [N/L], stencil tensor [G, taps + 1], keys) of a noise-model dict on DeviceOps
    ``ops``: groups from ``ground_groups`` ((observation, feed), which must each be one run of
    offsets), group g's stencil = its largest sample weight times ``noise_prior_stencil`` of its
    (fknee, alpha): model['fknee'] / ['alpha'] for every group, or model['table'] {(obsid, feed):
    (fknee, alpha)} per group.  A group without a valid model (absent, not finite, fknee <= 0 or
    alpha >= 0) or without a non-zero weight (a flagged feed) gets no prior (id -1).  keys: the
    (obsid, feed) pairs this rank holds."""
    torch = ops.torch
    taps = int(model.get('taps', 16))
    gid, uobs, ufeed = ground_groups(model['feedid'], model['obsids'], offset_length)
    G = uobs.size * ufeed.size
    held = np.unique(gid)
    keys = [(int(uobs[g // ufeed.size]), int(ufeed[g % ufeed.size])) for g in held]
    table = model.get('table')
    # w-bar_g: the group's largest sample weight, from the weights on the device
    wbar = torch.zeros(max(G, 1), dtype=torch.float64, device=ops.dev)
    wbar.scatter_reduce_(0, torch.from_numpy(gid).to(ops.dev).to(torch.int64), ops.w[0].reshape(-1, ops.L).amax(dim=1),
                         reduce='amax', include_self=True)
    weighted = wbar.cpu().numpy() > 0
    t = np.zeros((max(G, 1), taps + 1))
    cache, valid = {}, np.zeros(max(G, 1), bool)
    for g, key in zip(held, keys):
        fk, al = table.get(key, (np.nan, np.nan)) if table is not None else (model['fknee'], model['alpha'])
        fk, al = float(fk), float(al)
        if not (weighted[g] and np.isfinite(fk) and np.isfinite(al) and fk > 0 and al < 0):
            continue
        if (fk, al) not in cache:
            cache[fk, al] = noise_prior_stencil(fk, al, offset_length, fs=float(model.get('fs', 50.0)), taps=taps)
        t[g], valid[g] = cache[fk, al], True
    gid = np.where(valid[gid], gid, -1).astype(np.int32)
    return gid, torch.from_numpy(t).to(ops.dev) * wbar[:, None], keys


_COPY_STREAMS = {}


def copy_stream(dev):
    """One side stream per device for the maps' device -> host copies, kept for the
    process: a torch.cuda.Stream created per problem cost the chain ~1 ms of idle GPU before
    its first CG kernel (the creation waits for the device, r04l trace)."""
    import torch
    key = torch.device(dev).index if not isinstance(dev, int) else dev
    cs = _COPY_STREAMS.get(key)
    if cs is None:
        cs = _COPY_STREAMS[key] = torch.cuda.Stream(dev)
    return cs


# The ground solve's driver across ranks when COMAP_DS_GROUND_SOLVE is not set: 'batched'
# (cg_solve_batched) or 'eager' (cg_solve).  Eager until the batched driver measures
# faster outside the rounds' spread: with two gloo ranks on one GPU it did at one observation per
# rank and did not at four; no multi-GPU figure exists yet.
GROUND_RANKS_SOLVE = 'eager'

TILE = 8     # map layout tile (pixels per side) for a known map shape; COMAP_DS_TILE=0: row-major


_LAYOUTS = {}


def tiled_layout(ny, nx, T, device):
    """Internal id of every row-major pixel of an ny x nx map on a 2-D tiled layout: T x T
    tiles in row-major tile order, the pixels of a tile in Morton (Z) order; and the padded
    internal map size.  The operator then gathers 2-D neighbourhoods from shared cache lines
    and the set-up's spatial offset order (first pixel id) clusters offsets by tile (C5, 8
    obs: 1 band 0.139 -> 0.124, 4 bands 0.295 -> 0.275 ms per CG iteration with T = 8,
    scripts/ds_tiling_probe.py, profiles/r05/r05c_py2.log)."""
    import torch
    if T < 1 or T & (T - 1):
        raise ValueError(f'tile size must be a power of two, not {T}')
    key = (int(ny), int(nx), int(T), str(device))
    if key in _LAYOUTS:
        return _LAYOUTS[key]
    p = torch.arange(ny * nx, device=device, dtype=torch.int64)
    y, x = p // nx, p % nx
    ntx, nty = (nx + T - 1) // T, (ny + T - 1) // T
    ix, iy = x % T, y % T
    z = torch.zeros_like(p)
    for b in range(max(1, (T - 1).bit_length())):
        z |= ((ix >> b) & 1) << (2 * b)
        z |= ((iy >> b) & 1) << (2 * b + 1)
    ids = (((y // T) * ntx + x // T) * T * T + z).to(torch.int32)
    _LAYOUTS[key] = (ids, ntx * nty * T * T)
    return _LAYOUTS[key]


class DeviceDestriper:
    """Convenience wrapper: the whole destriper_iteration on device tensors.

    One band ([N] tod/weights): solve() -> {'x': [N/L], 'iters': int,
    'maps': {k: [npix]}}.  Several bands ([n_bands, N], one batched system):
    {'x': [n_bands, N/L], 'iters': [per band], 'maps': {k: [n_bands, npix]}}.

    Across ranks (torch.distributed initialised, world > 1) every rank passes its own
    samples and gets its own offsets and the full maps.  The problem is either
    sharded (each rank's operator, RCCL all-reduces every CG iteration) or gathered
    to rank 0, which solves it alone and hands back each rank's offsets and the maps:
    mapmaking/rankplan.py models both (COMAP_DS_RANKS=auto: small problems such as one
    observation (C4) are latency-bound across ranks and are gathered, large ones (C5)
    sharded).  The default is COMAP_DS_RANKS=shard until a multi-GPU run replaces the
    model's assumed all-reduce latency and bandwidth; gather forces the other.

    With ``ground=`` across ranks the problem is always sharded, whatever COMAP_DS_RANKS says
    (``gather`` and ``auto`` are not supported with the ground template; a ``gather`` request
    falls back to shard with a warning): every rank must hold whole (observation, feed)
    groups, whose offsets, slopes and levels are then rank-local unknowns.

    With ``split=`` across ranks the problem is always sharded too (``gather`` warns and shards,
    ``auto`` is ignored): each rank bins its own samples with its own offsets and the sums are
    added across ranks.  The same holds with ``residuals=`` / ``residual_cut=``: each rank's
    residual pass runs on its own samples and offsets against the global map, the group sums and
    counts are added across ranks, and every rank takes the same cut."""

    def __init__(self, pixels, tod, weights, offset_length, npix, device=None, keep=None, map_shape=None,
                 ground=None, split=None, residuals=None, residual_groups=None, residual_cut=None, prior=None,
                 solve_mask=None):
        """map_shape (ny, nx): the map's row-major layout (CAR / WCS maps), when known; the
        operator then runs on a 2-D tiled internal pixel order (tiled_layout) and the maps
        come back in the caller's order.
        ground (az, feedid, obsids), per sample: also fit an azimuth slope and a level per
        (observation, feed) jointly with the offsets (GroundOps; the reference's
        op_Ax_with_ground, Destriper.py:265-336).  solve() then adds res['ground'].  One band.
        The fit is per file and feed, hence local to the rank that holds the file: across ranks
        every (observation, feed) must lie on one rank (ValueError on every rank otherwise, as
        for any rank's set-up error), and rank 0's res['ground'] is the merged table of all
        ranks (merge_ground_tables; None on the others).
        split (labels, n_labels): also bin per-label maps of tod - F x with the solve's own
        offsets (the reference's "Create individual feed maps too" block, Destriper.py:487-501;
        comap_destripe_split_maps): ``labels`` holds one int32 per offset in [-1, n_labels), -1
        leaving the offset out of every split (``split_labels`` makes them by feed or by
        observation; across ranks label g must mean the same on every rank).  solve() then adds
        res['splits'] = {'map', 'naive', 'weight', 'hits'}, each [n_labels, npix] (one band) or
        [n_bands, n_labels, npix], in the caller's pixel order.  A list of such pairs gives a
        list of such dicts.  Not with ``ground``: the residual would need the fitted template
        per sample.
        residuals: True -- one group per (observation, feed), from residual_groups=(feedid,
        obsids) per sample (``residual_group_labels``) -- or (gid, n_groups), one int32 label per
        offset in [-1, n_groups), -1 = in no group: after the solve, the residual chi-squared of
        tod - F x - P m per group (comap_destripe_residuals; across ranks each rank's own samples
        and offsets against the global map, the group sums added over ranks).  solve() then adds
        res['residuals'] = {'chi2', 'sum', 'count'} ([n_groups] or [n_bands, n_groups]; chi2 =
        sum / count where count > 0, else 0) and {'offset_sum', 'offset_count'} ([N/L] or
        [n_bands, N/L], this rank's offsets).  A non-finite tod makes its group's chi2 NaN.
        residual_cut c (a float; implies residuals): group g of band b is cut when count > 0 and
        not chi2 <= c (so a NaN is cut); if any is, the operator is rebuilt with the cut groups'
        weights zeroed and their offsets dropped (keep 0: they leave the hit map), solved ONCE
        more (not iterated) and the residuals recomputed; res['residuals'] gains 'cut' (bool) and
        'chi2_first' (the first pass's chi2).  Not with ``ground`` either.
        prior: a noise prior on the offsets, (A + T) x = b (PriorOps; off by default) -- (gid,
        stencil), one int32 group id per offset in [-1, G) (-1: no prior; every group one
        contiguous run of offsets) and float64 [G, K + 1]; or a noise model {'fknee', 'alpha'[,
        'taps': 16], 'feedid', 'obsids'} (or 'table': {(obsid, feed): (fknee, alpha)} in place of
        the two values), whose groups are ``ground_groups``' and whose stencils are the group's
        largest weight times ``noise_prior_stencil`` (``prior_from_model``).  One band, not with
        ``ground``.  On one rank the solve is native (COMAP_DS_PRIOR_SOLVE=eager: ``cg_solve`` on
        PriorOps); across ranks the problem is always sharded and every group must lie whole on
        one rank (ValueError on every rank otherwise), so T is rank-local.  ``split`` and
        ``residuals`` work with it: they only consume x.
        solve_mask: a solve mask (MADAM's "inmask"; off by default) -- one flag per map pixel in the
        caller's pixel order, bool / integer / float [npix] or, with ``map_shape``, [ny, nx];
        non-zero = masked.  The offsets are fitted from the samples outside the masked pixels (w' =
        0 on them; off-map samples keep their weight), on a view of the problem
        (DeviceOps.masked_view: ``self.sops``); the maps, split maps and residuals then use every
        sample with its full weight and those offsets (``self.ops``).  An offset wholly inside
        the mask stays 0 -- or, with ``prior``, is carried across by its neighbours.  solve()
        adds res['solve_mask'] = {'pixels', 'samples', 'empty_offsets'} (the masked pixels, and per
        band the weighted samples masked and the offsets left without data, over all ranks).
        Works with ``prior``, ``split``, ``residuals`` and batched bands; across ranks the problem
        is always sharded.  Not with ``ground`` or ``residual_cut``.  ``set_solve_mask`` replaces
        or removes the mask on the built problem."""
        self.layout, self.okey = None, None
        self.prior, self.pops = None, None
        self.mask_info, self.map_shape, self.sops = None, map_shape, None
        _prior_check(prior, ground, np.ndim(tod) == 2 if not hasattr(tod, 'dim') else tod.dim() == 2)
        _mask_check(solve_mask, ground, residual_cut)
        self.npix_caller = int(npix)
        self.ground = None
        self.split = None
        self.resid, self.resid_cut, self.resid_axes = None, None, None
        if split is not None and ground is not None:
            raise NotImplementedError('split maps with the ground template are not supported')
        if residual_cut is not None and residuals is None:
            residuals = True
        if residuals is False:
            residuals = None
        if residuals is not None and ground is not None:
            raise NotImplementedError('residuals with the ground template are not supported: the residual '
                                      'would need the fitted template per sample')
        if residuals is True and residual_groups is None:
            raise ValueError('residuals=True needs residual_groups=(feedid, obsids)')
        T = int(os.environ.get('COMAP_DS_TILE', str(TILE)))
        if T > 0 and T & (T - 1):
            # the Morton code inside a tile interleaves log2(T) bits: for another T it would
            # exceed T * T - 1 and merge distinct pixels of neighbouring tiles
            raise ValueError(f'COMAP_DS_TILE must be 0 (row-major) or a power of two, not {T}')
        if map_shape is not None and T > 0:
            ny, nx = (int(v) for v in map_shape)
            if ny * nx != int(npix):
                raise ValueError(f'map_shape {map_shape} does not hold {npix} pixels')
            pixels, npix = self._tile(pixels, int(npix), ny, nx, T, device, int(offset_length))
        self.npix_full, self.hit_index = int(npix), None
        self.multi = np.ndim(tod) == 2 if not hasattr(tod, 'dim') else tod.dim() == 2
        self.gathered, self.plan = None, None
        d = _dist()
        if ground is not None:
            if self.multi:
                raise NotImplementedError('the ground template solves one band: pass a 1-D tod')
        ranks = d is not None and d.get_world_size() > 1
        if ranks and os.environ.get('COMAP_DS_RANKS', 'shard') == 'gather':
            import warnings
            for asked, what in ((ground, 'the ground template'), (split, 'split maps'), (residuals, 'residuals'),
                                (prior, 'the noise prior'), (solve_mask, 'a solve mask')):
                if asked is not None:
                    warnings.warn(f'COMAP_DS_RANKS=gather is not supported with {what}: sharding')
        if ranks:
            if ground is None and split is None and residuals is None and prior is None and solve_mask is None \
                    and self._choose_gather(d, pixels, tod, offset_length):
                self._gather(d, pixels, tod, weights, keep, offset_length, npix, device)
                return
            if os.environ.get('COMAP_DS_COMPACT', '1') != '0':
                pixels, npix = self._compact(pixels, int(npix), device)
        self.ops = N.retry_oom(DeviceOps, pixels, tod, weights, offset_length, npix, device, keep, self.okey)
        self.sops = self.ops                        # the problem the CG solves (a view under a solve mask)
        if solve_mask is not None:
            self._mask_view(solve_mask)
        if residuals is not None:
            self.resid_cut = None if residual_cut is None else float(residual_cut)
            if residuals is True:
                gid, uobs, ufeed = residual_group_labels(*residual_groups, offset_length)   # (fails on every rank)
                self.resid_axes = (uobs, ufeed)
                residuals = (gid, uobs.size * ufeed.size)
            # (a rank's bad labels, like any local set-up error below, must fail every rank)
            self.resid, _ = _on_every_rank('residuals', lambda: self._labels(*residuals, 'residual group'))
        if split is not None:
            # self.split_single: the caller passed one (labels, n_labels) pair, not a list
            self.split_single = isinstance(split, tuple)
            pairs = [split] if self.split_single else split
            self.split, _ = _on_every_rank('split maps', lambda: [self._labels(*p, 'split', True) for p in pairs])
        if ground is not None:
            az, feedid, obsids = ground

            def set_up():
                gid, uobs, ufeed = ground_groups(feedid, obsids, offset_length)
                self.ground = (uobs, ufeed)
                self.held = (np.bincount(gid, minlength=uobs.size * ufeed.size) > 0).reshape(uobs.size, ufeed.size)
                self.gops = N.retry_oom(GroundOps, self.ops, az, gid, uobs.size * ufeed.size)
                return {'obsids': uobs, 'feeds': ufeed, 'held': self.held}

            _, tables = _on_every_rank('ground template set-up', set_up, (ValueError, IndexError), lambda t: t)
            if tables is not None:
                merge_ground_tables(tables)     # two ranks holding one (observation, feed) fails on every rank
        if prior is not None:
            def set_up():
                if isinstance(prior, dict):
                    gid, stencil, keys = prior_from_model(self.ops, prior, int(offset_length))
                else:
                    gid, stencil = prior
                    g = gid.cpu().numpy() if hasattr(gid, 'cpu') else np.asarray(gid)
                    keys = [int(v) for v in np.unique(g[g >= 0])]
                self.pops = N.retry_oom(PriorOps, self.sops, gid, stencil)
                self.prior = (self.pops.gid, self.pops.stencil)
                return keys

            _, held = _on_every_rank('noise prior set-up', set_up, (ValueError, IndexError), lambda k: k)
            if held is not None:
                # (T is rank-local only when every group lies whole on one rank)
                seen = {}
                for rank, keys in enumerate(held):
                    for k in keys:
                        if k in seen:
                            raise ValueError(f'noise prior: group {k} has offsets on ranks {seen[k]} and {rank}: '
                                             'every group must lie on one rank')
                        seen[k] = rank

    def _mask_view(self, solve_mask):
        """self.sops = the view of self.ops under ``solve_mask`` (the caller's pixel order), and
        self.mask_info; a rank's bad mask fails on every rank."""
        ops = self.ops
        torch = ops.torch

        def set_up():
            flags = solve_mask_flags(solve_mask, self.npix_caller, self.map_shape)
            m = torch.from_numpy(flags).to(ops.dev)
            if self.layout is not None:             # onto the tiled layout (padding pixels unmasked)
                t = torch.zeros(self.npix_full, dtype=torch.uint8, device=ops.dev)
                t[self.layout.to(torch.int64)] = m
                m = t
            if self.hit_index is not None:          # a mask pixel the compaction dropped is simply unused
                m = m[self.hit_index]
            return m.contiguous(), flags

        (m, flags), _ = _on_every_rank('solve mask', set_up)
        self.sops = N.retry_oom(ops.masked_view, m)
        # what the mask took, per band: weighted samples on masked pixels, offsets left without any
        on = (ops.pix >= 0) & (m[ops.pix.clamp(min=0).to(torch.int64)] != 0)
        had = (ops.w != 0)
        gone = had & on[None, :]
        left = (had & ~on[None, :]).reshape(ops.nb, ops.n_offsets, ops.L).any(dim=2)
        empty = had.reshape(ops.nb, ops.n_offsets, ops.L).any(dim=2) & ~left
        counts = torch.stack([gone.sum(dim=1), empty.sum(dim=1)]).to(torch.int64)
        torch_allreduce(counts)
        counts = counts[:, :ops.n_bands].cpu().numpy()
        one = (lambda v: int(v[0])) if not self.multi else (lambda v: v.copy())
        self.mask_info = {'pixels': int(flags.sum()), 'samples': one(counts[0]), 'empty_offsets': one(counts[1])}
        self.mask_flags = flags

    def set_solve_mask(self, solve_mask):
        """Replace the solve mask (None: remove it) on the built problem: only the view is rebuilt
        -- the parent problem, the split and residual labels and the prior's stencils stay; with
        a prior its handle is re-created on the new view."""
        _mask_check(solve_mask, self.ground, self.resid_cut)
        if self.gathered is not None:
            raise NotImplementedError('a solve mask on a gathered problem is not supported: build with solve_mask')
        self.pops = None                            # (the prior's handle borrows the view)
        self.sops = self.ops
        self.mask_info = None
        if solve_mask is not None:
            self._mask_view(solve_mask)
        if self.prior is not None:
            self.pops = N.retry_oom(PriorOps, self.sops, *self.prior)

    def _labels(self, labels, n_labels, what, times_npix=False):
        """(int32 CUDA labels [N/L], n_labels) of a split ('split') or of the residual groups;
        host labels are range-checked here, device labels by the pass itself (ValueError either
        way).  times_npix: n_labels * npix must fit 31 bits too (the split maps' key)."""
        torch = self.ops.torch
        G = int(n_labels)
        if not isinstance(labels, torch.Tensor):
            labels = np.asarray(labels).reshape(-1)
            if labels.size and (int(labels.max()) >= G or int(labels.min()) < -1):
                raise ValueError(f'{what} label out of range (valid: -1 .. {G - 1})')
        t = self.ops._t(labels, torch.int32)
        if t.numel() != self.ops.n_offsets:
            raise ValueError(f'{what} labels: one per offset ({self.ops.n_offsets}), not {t.numel()}')
        if times_npix and (G < 1 or G * self.ops.npix >= 2 ** 31):
            raise ValueError(f'n_labels * npix must lie in [1, 2^31), not {G} * {self.ops.npix}')
        if G < 1:
            raise ValueError(f'{what}: n_groups must be >= 1, not {G}')
        return t, G

    def _split_maps(self, x):
        """res['splits'] (device tensors) for the solved offsets ``x`` ([N/L * nb], the caller's
        order): per requested split the rank's sums (DeviceOps.split_maps) added across ranks,
        divided, and laid out as the maps are: expanded from the compacted pixels, in the caller's
        pixel order, [n_labels, npix] or [n_bands, n_labels, npix]."""
        ops = self.ops
        out = []
        for labels, G in self.split:
            # (the pass itself checks device labels and pixel ids: across ranks its error must reach
            # every rank before the sums' all-reduce, where the other ranks would wait for this one)
            (num, nnum, weight, hits), _ = _on_every_rank('split maps', lambda: ops.split_maps(x, labels, G),
                                                          (ValueError, IndexError, N.NativeError))
            for v in (num, nnum, weight, hits):
                torch_allreduce(v)
            m, naive = ops.split_div(num, nnum, weight)
            out.append({k: self._split_layout(v, G) for k, v in zip(SPLIT_KEYS, (m, naive, weight, hits))})
        return out[0] if self.split_single else out

    def _splits_to_host(self, splits):
        """res['splits'] as host arrays on rank 0, None in their place on the other ranks."""
        d = _dist()
        rank = d.get_rank() if d is not None else 0
        sp = [maps_to_host(m) if rank == 0 else None for m in ([splits] if self.split_single else splits)]
        return sp[0] if self.split_single else sp

    def _split_layout(self, v, G):
        """[G * npix_internal * nb] (label, pixel, band fastest) -> [G, npix] (one band) or
        [n_bands, G, npix] in the caller's pixel order: _expand and _untile, every label at once."""
        ops = self.ops
        t = v.reshape(G, -1, ops.nb)
        if self.hit_index is not None:
            full = ops.torch.zeros((G, self.npix_full, ops.nb), dtype=v.dtype, device=v.device)
            full[:, self.hit_index] = t
            t = full
        if self.layout is not None:
            t = t.index_select(1, self.layout)
        if not self.multi:
            return t[:, :, 0].contiguous()
        return t.permute(2, 0, 1)[:ops.n_bands].contiguous()

    # ---- residual chi-squared
    def _bands(self, v):
        """[n * nb] interleaved table -> [n] (one band) or [n_bands, n]."""
        return self.ops.split_bands(v) if self.multi else v.reshape(-1, self.ops.nb)[:, 0].contiguous()

    def _residuals(self, x, m):
        """res['residuals'] (device tensors) for the solved offsets ``x`` ([N/L * nb], the caller's
        order) and the global map ``m`` ([npix_internal * nb], before _expand / _untile): the rank's
        pass (DeviceOps.residuals), the group sums and counts added across ranks -- with whole
        files per rank a group has one contributing rank, so the sum is exact."""
        torch = self.ops.torch
        # (the pass itself checks device labels and pixel ids: across ranks its error must reach
        # every rank before the all-reduce, where the other ranks would wait for this one)
        (off_sum, off_cnt, grp_sum, grp_cnt), _ = _on_every_rank(
            'residuals', lambda: self.ops.residuals(x, m, *self.resid), (ValueError, IndexError, N.NativeError))
        torch_allreduce(grp_sum)
        torch_allreduce(grp_cnt)
        s, c = self._bands(grp_sum), self._bands(grp_cnt)
        chi2 = torch.where(c > 0, s / torch.where(c > 0, c, torch.ones_like(c)).to(torch.float64), torch.zeros_like(s))
        return {'chi2': chi2, 'sum': s, 'count': c, 'offset_sum': self._bands(off_sum),
                'offset_count': self._bands(off_cnt)}

    def _cut_groups(self, cut):
        """The operator rebuilt without the cut groups (``cut`` bool [n_bands, G] or [G]): band
        b's weights zeroed on every sample of its cut groups and keep[b][o] = 0 on their offsets."""
        ops = self.ops
        torch = ops.torch
        gid, G = self.resid
        nbo, NO, L = ops.n_bands, ops.n_offsets, ops.L
        cut2 = cut.reshape(nbo, G)
        idx = gid.to(torch.int64).clamp(min=0)
        gone = cut2[:, idx] & (gid >= 0)[None, :]                           # [n_bands, N/L]
        w = ops.w[:nbo].clone()
        w.view(nbo, NO, L)[gone] = 0.0
        keep = torch.ones((nbo, NO), dtype=torch.uint8, device=ops.dev) if ops.keep is None else ops.keep[:nbo].clone()
        keep[gone] = 0
        pix, tod, npix, dev = ops.pix, ops.tod[:nbo], ops.npix, ops.dev.index
        self.pops = None                                                    # (the prior's handle borrows the problem)
        self.ops = None                                                     # (the old problem's buffers go first)
        del ops
        self.ops = N.retry_oom(DeviceOps, pix, tod, w, L, npix, dev, keep, self.okey)
        self.sops = self.ops                                                # (no solve mask with a cut: _mask_check)
        if self.prior is not None:                                          # the same prior on the rebuilt operator
            self.pops = N.retry_oom(PriorOps, self.ops, *self.prior)

    def solve(self, threshold=1e-6, niter=100, to_host=False, allreduce=None):
        """to_host: maps as host NumPy arrays (rank 0; None on the others) -- one
        rank solving alone overlaps their copy with the CG (solve_native_host).
        allreduce: the sharded CG's sum across ranks (default torch_allreduce; bench.py
        passes a TimedAllreduce to measure the per-iteration collective cost).
        With ``residual_cut`` the solve runs a second time when the first pass cut a group."""
        res = self._solve(threshold, niter, to_host, allreduce)
        if self.resid is None or self.resid_cut is None:
            return res
        torch = self.ops.torch
        r = res['residuals']
        chi2, count = (torch.as_tensor(r[k]) for k in ('chi2', 'count'))
        cut = (count > 0) & ~(chi2 <= self.resid_cut)                       # (a NaN chi2 is cut)
        if bool(cut.any()):
            self._cut_groups(cut.to(self.ops.dev))
            res = self._solve(threshold, niter, to_host, allreduce)
        conv = (lambda v: v.cpu().numpy()) if to_host else (lambda v: v)
        res['residuals'].update(cut=conv(cut), chi2_first=conv(chi2))
        return res

    # ---- rank policy
    def _choose_gather(self, d, pixels, tod, offset_length):
        import torch
        from . import rankplan
        # default 'shard': the rank model's all-reduce latency / ring bandwidth are assumptions
        # until a multi-GPU run measures them (rankplan.py), so 'auto' is opt-in
        policy = os.environ.get('COMAP_DS_RANKS', 'shard')
        if policy == 'shard':
            return False
        n_local = int(pixels.numel()) if hasattr(pixels, 'numel') else int(np.size(pixels))
        n_bands = (int(tod.shape[0]) if self.multi else 1)
        dev = self._comm_device(d)
        cnt = torch.tensor([n_local], dtype=torch.int64, device=dev)
        parts = [torch.zeros_like(cnt) for _ in range(d.get_world_size())]
        d.all_gather(parts, cnt)
        self.counts = [int(c.item()) for c in parts]
        if policy == 'gather':
            return True
        self.plan = rankplan.plan(sum(self.counts), n_bands, d.get_world_size())
        return self.plan['mode'] == 'gather'

    @staticmethod
    def _comm_device(d):
        import torch
        return torch.device('cuda', torch.cuda.current_device()) if d.get_backend() == 'nccl' else torch.device('cpu')

    def _gather(self, d, pixels, tod, weights, keep, offset_length, npix, device):
        """Inputs of every rank to rank 0 (padded to the largest rank, in rank order);
        rank 0 builds the single-rank operator on their concatenation."""
        import torch
        L = int(offset_length)
        rank, world = d.get_rank(), d.get_world_size()
        cdev = self._comm_device(d)
        nbands = int(tod.shape[0]) if self.multi else 1
        nmax = max(self.counts)

        def as_t(a, dt):
            return _to_tensor(a, cdev, dt)

        def gather(t, width):       # t [rows, n_local] -> root: list of [rows, width]
            pad = torch.zeros((t.shape[0], width), dtype=t.dtype, device=cdev)
            pad[:, :t.shape[1]] = t
            parts = [torch.zeros_like(pad) for _ in range(world)] if rank == 0 else None
            d.gather(pad, gather_list=parts, dst=0)
            return parts

        pix = gather(as_t(pixels, torch.int32).reshape(1, -1), nmax)
        td = gather(as_t(tod, torch.float64).reshape(nbands, -1), nmax)
        wd = gather(as_t(weights, torch.float64).reshape(nbands, -1), nmax)
        kp = None
        if keep is not None:
            kp = gather(as_t(keep, torch.uint8).reshape(nbands, -1), nmax // L)
        self.gathered = {'counts': self.counts, 'L': L}
        if rank != 0:
            self.ops = None
            self._ref = (device, nbands)
            return
        dev = _device(device)
        cat = lambda parts, per: torch.cat([parts[r][:, :c // per] for r, c in enumerate(self.counts)], dim=1).to(dev)  # noqa: E731
        p_all, t_all, w_all = cat(pix, 1).reshape(-1), cat(td, 1), cat(wd, 1)
        k_all = cat(kp, L) if kp is not None else None
        if not self.multi:
            t_all, w_all = t_all.reshape(-1), w_all.reshape(-1)
        self.ops = DeviceOps(p_all, t_all, w_all, L, npix, device, k_all)
        self._ref = (device, nbands)

    def _solve_gathered(self, d, threshold, niter):
        """Rank 0 solves; iterations and maps are broadcast, each rank's offsets sent back."""
        import torch
        rank, world = d.get_rank(), d.get_world_size()
        cdev = self._comm_device(d)
        device, nbands = self._ref
        nb = 4 if nbands == 3 else nbands
        L, counts = self.gathered['L'], self.gathered['counts']
        npix = self.npix_full
        dev = _device(device)
        nomax = max(counts) // L
        keys = ('map', 'naive', 'weight', 'hits')
        if rank == 0:
            x, it, maps = self.ops.solve_native(threshold, niter)
            its = torch.tensor(list(it) + [0] * (4 - len(it)), dtype=torch.int64, device=cdev)
            mp = torch.stack([maps[k] for k in keys]).to(cdev)
            xv = x.reshape(-1, nb)
            parts, o = [], 0
            for c in counts:
                pad = torch.zeros((nomax, nb), dtype=torch.float64, device=cdev)
                pad[:c // L] = xv[o:o + c // L]
                parts.append(pad)
                o += c // L
        else:
            its = torch.zeros(4, dtype=torch.int64, device=cdev)
            mp = torch.zeros((4, npix * nb), dtype=torch.float64, device=cdev)
            parts = None
        d.broadcast(its, src=0)
        d.broadcast(mp, src=0)
        mine = torch.zeros((nomax, nb), dtype=torch.float64, device=cdev)
        d.scatter(mine, scatter_list=parts, src=0)
        x = mine[:counts[rank] // L].reshape(-1).to(dev)
        it = [int(v) for v in its.cpu()][:nbands]
        maps = {k: mp[i].to(dev) for i, k in enumerate(keys)}
        return x, it, maps, nb, nbands

    def _tile(self, pixels, npix, ny, nx, T, device, L):
        """Relabel the pixel ids onto tiled_layout; a negative id p (an unbinned sample that
        reads m[npix + p]) becomes the negative id that reads the same pixel there.  With
        COMAP_DS_OKEY=centroid (default) the offsets are also ordered by their centroid
        pixel's internal id (comap_offset_centroid_keys) instead of their first pixel: the
        offsets crossing one pixel then sit close together, which is what the CG bin's x
        gathers touch."""
        import torch
        dev = _device(device)
        pix = _to_tensor(pixels, dev, torch.int32).reshape(-1)
        ids, nt = tiled_layout(ny, nx, T, dev)
        # one device pass (comap_relabel_pixels), no host sync: an id outside [-npix, npix)
        # becomes nt, which the set-up's device range check rejects (IndexError), as it
        # would the original id
        out = torch.empty_like(pix)
        c = N.ctx(dev.index)
        N.bind_stream(c, dev)
        N.check(N.lib().comap_relabel_pixels_tiled(c, N.dptr(pix), pix.numel(), int(nx), int(ny), int(T),
                                                   N.dptr(out)), c, 'comap_relabel_pixels_tiled')
        if os.environ.get('COMAP_DS_OKEY', 'centroid') == 'centroid' and pix.numel() % L == 0:
            keys = torch.empty(pix.numel() // L, dtype=torch.int32, device=dev)
            N.check(N.lib().comap_offset_centroid_keys(c, N.dptr(pix), pix.numel(), int(L), int(nx), int(ny),
                                                       N.dptr(ids), int(nt), N.dptr(keys)), c,
                    'comap_offset_centroid_keys')
            self.okey = (keys, int(nt) + 1)
        self.layout = ids
        return out, nt

    def _untile(self, v, nb):
        """[npix_internal * nb] interleaved map -> the caller's row-major [npix * nb]."""
        if self.layout is None:
            return v
        return v.reshape(-1, nb).index_select(0, self.layout).reshape(-1)   # (int32 ids)

    def _compact(self, pixels, npix, device):
        """Across ranks the map numerator is all-reduced every CG iteration
        (Destriper.py:183-204); only pixels some rank's samples hit can be non-zero.
        Relabel the pixels onto that union, in increasing pixel order, so every
        all-reduce carries the hit pixels only ("compact to hit pixels").
        The relabelling is monotone, and the pixels that unbinned samples read are kept
        (a negative id p reads m[npix + p], Destriper.py:206-213): the per-pixel sums, the
        offsets' spatial order and hence every iterate are unchanged, bit for bit.  Maps are
        expanded back to npix in solve()."""
        import torch
        pix = _to_tensor(pixels, _device(device), torch.int64).reshape(-1)
        if pix.numel() and (int(pix.max().item()) >= npix or int(pix.min().item()) < -npix):
            raise IndexError(f'pixel index out of range for a map of {npix} pixels (valid: -{npix} .. {npix - 1})')
        comp, self.hit_index = compact_pixels(pix, npix, torch_allreduce)
        return comp, int(self.hit_index.numel())

    def _expand(self, v):
        """[n_hit * nb] interleaved map on the compacted pixels -> [npix * nb]."""
        if self.hit_index is None:
            return v
        nb = self.ops.nb
        out = self.ops.torch.zeros((self.npix_full, nb), dtype=v.dtype, device=v.device)
        out[self.hit_index] = v.reshape(-1, nb)
        return out.reshape(-1)

    def nnz(self):
        return self.ops.nnz()

    def entry_bytes(self):
        return self.ops.entry_bytes()

    def sell_entries(self):
        return self.ops.sell_entries()

    def _solve(self, threshold, niter, to_host, allreduce):
        """One solve() of the problem as it stands (see solve).  With residuals the single-rank
        to_host call takes the general path: the overlapped solve_native_host never leaves the
        device map in reach."""
        if self.ground is not None:
            return self._solve_ground(threshold, niter, to_host)
        d = _dist()
        ops = self.ops                              # the full problem ...
        sops = ops if self.sops is None else self.sops      # ... and the one the CG solves (its view under a mask)
        if to_host and self.gathered is None and (d is None or d.get_world_size() == 1) and self.resid is None \
                and self.prior is None:
            x, it, maps = sops.solve_native_host(threshold, niter, unmap=self.layout)
            maps['map2'] = maps['weight']
            if not self.multi:
                res = {'x': x, 'iters': it[0], 'maps': {k: v[0] for k, v in maps.items()}}
            else:
                res = {'x': ops.split_bands(x), 'iters': it, 'maps': maps}
            if self.split is not None:           # after the overlapped solve, on the device x
                res['splits'] = self._splits_to_host(self._split_maps(x))
            if self.mask_info is not None:
                res['solve_mask'] = dict(self.mask_info)
            return res
        if to_host:
            res = self._solve(threshold, niter, False, None)
            rank = d.get_rank() if d is not None else 0
            res['maps'] = maps_to_host(res['maps']) if rank == 0 else None
            if self.resid is not None:           # (small, and the same on every rank: host arrays everywhere)
                res['residuals'] = {k: v.cpu().numpy() for k, v in res['residuals'].items()}
            if self.split is not None:
                res['splits'] = self._splits_to_host(res['splits'])
            return res
        if self.gathered is not None:
            x, it, maps, nb, nbands = self._solve_gathered(d, threshold, niter)
            split = lambda v: v.reshape(-1, nb).t()[:nbands].contiguous()   # noqa: E731
        elif self.prior is not None:
            # one rank: the native solve (COMAP_DS_PRIOR_SOLVE=eager: Python's cg_solve on PriorOps);
            # across ranks cg_solve with the sharded all-reduces, T being rank-local
            ranks = d is not None and d.get_world_size() > 1
            mode = os.environ.get('COMAP_DS_PRIOR_SOLVE', 'native')
            if mode not in ('native', 'eager'):
                raise ValueError(f"COMAP_DS_PRIOR_SOLVE must be 'native' or 'eager', not {mode!r}")
            if ranks or mode == 'eager':
                x, it, h, nnum = cg_solve(self.pops, (allreduce or torch_allreduce) if ranks else (lambda t: t),
                                          threshold, niter)
                maps, m_internal = self._finish_maps(ops, x, h, nnum)
                x, it = ops.natural(x), [it]
            else:
                x, it, maps = self.pops.solve_native(threshold, niter)
                m_internal = maps['map']
            split = ops.split_bands
        elif d is None or d.get_world_size() == 1:
            x, it, maps = sops.solve_native(threshold, niter)
            split = ops.split_bands
            m_internal = maps['map']
        else:
            # COMAP_DS_GRAPH=1: the captured-graph driver (one launch per 16 iterations);
            # default: the eager batched driver (4 native calls and 3 all-reduces per iteration,
            # 16 iterations per check)
            # (graph capture of a collective needs RCCL: with any other backend, e.g. the gloo
            # rehearsals, the eager driver runs instead)
            solver = cg_solve_batched
            if os.environ.get('COMAP_DS_GRAPH') == '1':
                if d.get_backend() == 'nccl':
                    solver = cg_solve_graph
                else:
                    import warnings
                    warnings.warn(f'COMAP_DS_GRAPH=1 needs the nccl (RCCL) backend, not {d.get_backend()}: '
                                  'using the eager CG driver')
            x, it, h, nnum = solver(sops, allreduce or torch_allreduce, threshold, niter)
            maps, m_internal = self._finish_maps(ops, x, h, nnum)
            it = it[:ops.n_bands]
            x = ops.natural(x)
            split = ops.split_bands
        if self.layout is not None:
            nbl = nb if self.gathered is not None else ops.nb
            maps = {k: self._untile(v, nbl) for k, v in maps.items()}
        extra = {} if self.split is None else {'splits': self._split_maps(x)}
        if self.resid is not None:
            extra['residuals'] = self._residuals(x, m_internal)
        if self.mask_info is not None:
            extra['solve_mask'] = dict(self.mask_info)
        if not self.multi:
            maps['map2'] = maps['weight']
            return {'x': x, 'iters': it[0], 'maps': maps, **extra}
        maps = {k: split(v) for k, v in maps.items()}
        maps['map2'] = maps['weight']
        return {'x': split(x), 'iters': it, 'maps': maps, **extra}

    def _finish_maps(self, op, u, h, nnum):
        """The device maps {'map', 'naive', 'weight', 'hits'} of solution ``u`` of operator ``op``
        (self.ops or self.gops: op.bin(u, 1, num) is the rank's naive numerator - W u), from the
        global weight map h and naive numerator nnum: hits and the numerator summed across
        ranks, divided by h and expanded to the full map; and the map as it is before that, on
        the problem's internal (compacted) pixels, which the residual pass reads."""
        ops = self.ops
        n = ops.npix * ops.nb
        h0, hits, n0 = ops.local_maps()
        torch_allreduce(hits)
        if self.sops is not ops:                    # a solve mask: the CG's h and nnum are the view's
            h, nnum = torch_allreduce(h0), torch_allreduce(n0)
        num = ops.zeros(n)
        op.bin(u, 1, num)
        torch_allreduce(num)
        maps = {'map': ops.zeros(n), 'naive': ops.zeros(n), 'weight': h, 'hits': hits}
        ops.div_map(num, h, maps['map'])
        ops.div_map(nnum, h, maps['naive'])
        return {k: self._expand(v) for k, v in maps.items()}, maps['map']

    def _solve_ground(self, threshold, niter, to_host):
        """solve() with the ground template, then the maps from the offsets AND the fitted
        templates.  COMAP_DS_GROUND_SOLVE, read here, picks the CG: on one rank 'native' (the
        default: ``GroundOps.solve_native``, device-resident) or 'eager' (Python's ``cg_solve``,
        the comparison baseline); across ranks (sharded, on the rank's own groups) 'eager' with
        the sharded all-reduces (the default, GROUND_RANKS_SOLVE) or 'batched' (= 'native':
        ``cg_solve_batched``, device stop test, 16 iterations per host check; the same iterates
        bit for bit), the maps then from the all-reduced numerator, hits and global weight map.
        Adds 'ground': {'obsids', 'feeds', 'slope', 'level', 'wrapped'} (host arrays [n_obs,
        n_feeds], GroundOps.fit's units; 'wrapped': the group crosses azimuth 0 / 360 and was
        fitted on az + 360 where az < 180): across ranks the merged table on rank 0, None
        elsewhere.  'x' holds the rank's offsets, 'solution' its whole CG vector [x internal
        order | s | c] in GroundOps' units."""
        ops, g = self.ops, self.gops
        d = _dist()
        ranks = d is not None and d.get_world_size() > 1
        mode = os.environ.get('COMAP_DS_GROUND_SOLVE', GROUND_RANKS_SOLVE if ranks else 'native')
        if mode == 'eager':
            u, it, h, nnum = cg_solve(g, torch_allreduce, threshold, niter)
        elif ranks and mode in ('batched', 'native'):
            u, its, h, nnum = cg_solve_batched(g, torch_allreduce, threshold, niter)
            it = its[0]
        elif mode == 'native':
            u, it, maps = g.solve_native(threshold, niter)
        else:
            raise ValueError("COMAP_DS_GROUND_SOLVE must be 'native', 'eager' or, across ranks, 'batched', "
                             f'not {mode!r}')
        if ranks or mode == 'eager':
            maps, _ = self._finish_maps(g, u, h, nnum)
        if self.layout is not None:
            maps = {k: self._untile(v, 1) for k, v in maps.items()}
        maps['map2'] = maps['weight']
        uobs, ufeed = self.ground
        slope, level = (v.cpu().numpy().reshape(uobs.size, ufeed.size) for v in g.fit(u))
        table = {'obsids': uobs, 'feeds': ufeed, 'slope': slope, 'level': level,
                 'wrapped': g.wrapped.cpu().numpy().reshape(uobs.size, ufeed.size) != 0}
        rank = 0
        if ranks:
            tables = [None] * d.get_world_size()
            d.all_gather_object(tables, dict(table, held=self.held))
            rank = d.get_rank()
            table = merge_ground_tables(tables) if rank == 0 else None
        if to_host:
            maps = maps_to_host(maps) if rank == 0 else None
        return {'x': ops.natural(u), 'iters': it, 'maps': maps, 'ground': table, 'solution': u}


def maps_to_host(maps):
    """{name: device tensor} -> {name: NumPy array}: one device-side stack and one copy
    into page-locked host memory from the library's cache (a pageable copy per map runs
    at a fraction of the link)."""
    import torch
    keys = list(maps)
    if not keys:
        return {}
    flat = torch.stack([maps[k].reshape(-1) for k in keys])
    a = N.host_empty(tuple(flat.shape), str(flat.dtype).split('.')[-1])    # cached page-locked block
    torch.from_numpy(a).copy_(flat, non_blocking=True)
    torch.cuda.current_stream(flat.device).synchronize()
    return {k: a[i].reshape(tuple(maps[k].shape)) for i, k in enumerate(keys)}


def run_destriper(_pointing, _tod, _weights, offset_length, pixel_edges, az=None, el=None, ra=None, dec=None,
                  feedid=None, obsids=None, obsid_cuts=None, threshold=1e-6, niter=100, chi2_cutoff=100,
                  special_weight=None, healpix=False, device=None, map_shape=None, ground=False, split=None,
                  residuals=False, residual_cut=None, prior=None, solve_mask=None):
    """Destriper.run_destriper (Destriper.py:456-503) on the GPU.

    ``pixel_edges[-1] + 1`` is the map size (bin_offset_map, :169).  Returns
    {'All': maps} with host NumPy maps on rank 0; other ranks get None maps.
    map_shape (ny, nx), an extension: the map's row-major layout, which lets the
    operator run on a 2-D tiled pixel order (DeviceDestriper).
    ground=True, an extension: fit an azimuth slope and a level per (observation, feed)
    from ``az``, ``feedid`` and ``obsids`` jointly with the offsets (the reference's
    op_Ax_with_ground, :265-336, which its run() leaves switched off); the result gains
    'Ground': {'obsids', 'feeds', 'slope', 'level', 'wrapped'}: across ranks (every
    (observation, feed) on one rank) rank 0 gets the merged table of all ranks' observations
    and the other ranks None maps and 'Ground': None.
    split='feed', 'obsid' or a list of these, an extension: the reference's commented "Create
    individual feed maps too" block (:487-501), completed -- one {'map', 'naive', 'weight',
    'hits'} entry per feed ('Feed01', ...) or observation ('Obs<obsid>') beside 'All', binned
    from that subset's samples of tod - F x with the solve's own offsets (None maps on ranks
    other than 0; across ranks the names are those of all ranks' feeds / observations), and
    'offsets', the rank's solved offsets (host, [N/L]).
    residuals=True and / or residual_cut=c, an extension (``chi2_cutoff`` and ``obsid_cuts`` stay
    ignored, as in the reference): the residual chi-squared of tod - F x - P m per (observation,
    feed) and, with a cut, one more solve without the groups above c (DeviceDestriper); the
    result gains 'Residuals': {'obsids', 'feeds', 'chi2', 'count'[, 'cut', 'chi2_first']}, tables
    [n_obs, n_feeds], on rank 0 and None on the other ranks.  Not together with ``ground``.
    prior, an extension (off by default): a noise prior on the offsets, DeviceDestriper's ``prior``
    -- (gid, stencil), or a noise model {'fknee', 'alpha'[, 'taps']} (or {'table': {(obsid, feed):
    (fknee, alpha)}}) that takes its groups from ``feedid`` and ``obsids``.  One band; not together
    with ``ground``.
    solve_mask, an extension (off by default): DeviceDestriper's ``solve_mask`` -- one flag per map
    pixel ([npix], or [ny, nx] with ``map_shape``); the offsets are fitted outside the masked pixels,
    the maps binned from every sample.  The result gains 'solve_mask': {'pixels', 'samples',
    'empty_offsets', 'mask'} ('mask': the flags, host uint8 [npix]).  ('snr', nsigma[, grow]) is the
    two-pass form, which needs ``map_shape``: a plain solve, ``mask_from_map`` of its map and weight map
    (rank 0's, handed to every rank), ``set_solve_mask`` on the same set-up and the solve again.  Not
    with ``ground``, ``residual_cut`` or ``healpix``."""
    _mask_check(solve_mask, ground, residual_cut, healpix)
    snr = _snr_spec(solve_mask)
    if snr is not None and map_shape is None:
        raise ValueError("solve_mask ('snr', ...) needs map_shape: the mask is grown on the 2-D map")
    _prior_check(None if prior is None else (dict(prior, feedid=feedid, obsids=obsids) if isinstance(prior, dict)
                                             else prior), ground, np.ndim(_tod) == 2)
    if isinstance(prior, dict):
        prior = dict(prior, feedid=feedid, obsids=obsids)
    if special_weight is not None:
        raise NotImplementedError('special_weight is unused by run_destriper in the reference (:482)')
    import torch
    if device is None:
        device = torch.cuda.current_device()
    npix = int(pixel_edges[-1]) + 1
    if ground and (az is None or feedid is None or obsids is None):
        raise ValueError('ground=True needs az, feedid and obsids')
    if ground and split:
        raise NotImplementedError('split maps with the ground template are not supported')
    resid = _residual_args(residuals, residual_cut, ground, feedid, obsids)
    specs = split_specs(split, feedid, obsids, offset_length)
    dd = DeviceDestriper(np.asarray(_pointing), np.asarray(_tod, dtype=np.float64),
                         np.asarray(_weights, dtype=np.float64), int(offset_length), npix, device, map_shape=map_shape,
                         ground=(np.asarray(az, dtype=np.float64), feedid, obsids) if ground else None,
                         split=None if specs is None else [(lab, len(names)) for lab, names in specs], prior=prior,
                         solve_mask=None if snr is not None else solve_mask, **resid)
    res = dd.solve(threshold, niter, to_host=True)
    if snr is not None:
        first = res['maps']
        ny, nx = (int(v) for v in map_shape)
        found = [None if first is None else mask_from_map(np.reshape(first['map'], (ny, nx)),
                                                          np.reshape(first['weight'], (ny, nx)), *snr)]
        d = _dist()
        if d is not None and d.get_world_size() > 1:
            d.broadcast_object_list(found, src=0)
        dd.set_solve_mask(found[0])
        res = dd.solve(threshold, niter, to_host=True)
    maps = res['maps']
    if maps is None:                     # a rank other than 0
        maps = {'map': None, 'naive': None, 'weight': None, 'map2': None}
    out = {'All': maps, 'Ground': res['ground']} if ground else {'All': maps}
    if solve_mask is not None:
        out['solve_mask'] = dict(res['solve_mask'], mask=dd.mask_flags)
    if resid:
        out['Residuals'] = _residual_table(dd, res['residuals'])
    if specs is not None:
        out.update(_split_entries(specs, res['splits']))
        out['offsets'] = res['x'].cpu().numpy()      # this rank's offsets, which its split maps were binned with
    return out


def _residual_args(residuals, residual_cut, ground, feedid, obsids):
    """The drivers' ``residuals`` / ``residual_cut`` as DeviceDestriper's keyword arguments
    ({} when neither is asked for)."""
    if not residuals and residual_cut is None:
        return {}
    if ground:
        raise NotImplementedError('residuals with the ground template are not supported')
    if feedid is None or obsids is None:
        raise ValueError('residuals need feedid and obsids')
    return {'residuals': True, 'residual_groups': (feedid, obsids), 'residual_cut': residual_cut}


def _residual_table(dd, r, band=None):
    """'Residuals' of a driver's result from res['residuals'] (host arrays; ``band``: of that
    band of a batched solve): tables [n_obs, n_feeds] on rank 0, None on the other ranks."""
    d = _dist()
    if d is not None and d.get_rank() != 0:
        return None
    uobs, ufeed = dd.resid_axes
    out = {'obsids': uobs, 'feeds': ufeed}
    for k in ('chi2', 'count', 'cut', 'chi2_first'):
        if k in r:
            v = np.asarray(r[k])
            out[k] = (v if band is None else v[band]).reshape(uobs.size, ufeed.size)
    return out


def _split_entries(specs, splits, band=None):
    """{name: {'map', 'naive', 'weight', 'hits'}} of every label of every requested split
    (``band``: of that band of a batched solve); None maps where the rank got none."""
    out = {}
    for (_, names), sp in zip(specs, splits):
        for g, name in enumerate(names):
            if sp is None:
                out[name] = dict.fromkeys(SPLIT_KEYS)
            else:
                out[name] = {k: (sp[k][g] if band is None else sp[k][band][g]) for k in SPLIT_KEYS}
    return out


def run_destriper_bands(_pointing, _tods, _weights, offset_length, pixel_edges, keep=None, threshold=1e-6,
                        niter=100, device=None, map_shape=None, split=None, feedid=None, obsids=None,
                        residuals=False, residual_cut=None, prior=None, solve_mask=None):
    """run_destriper for several sidebands on the same pointing in ONE batched
    device solve (the reference calls run_destriper once per band,
    run_destriper.py:146-189).  _tods/_weights [n_bands, N]; keep [n_bands, N/L]
    as returned by comapdata.read_comap_data_bands.  Returns one
    {'All': maps} per band (host maps on rank 0, None maps on other ranks);
    band b's maps and iteration count are those of run_destriper on band b's
    own samples, and its offsets (``x``, rank 0: also under 'offsets') cover
    the union of the bands' offsets (0 where band b dropped the offset).
    split ('feed', 'obsid' or a list of these, with per-sample ``feedid`` and ``obsids``): each
    band's dict also gets run_destriper's split-map entries, all bands' from one device pass
    per split; a band's 'hits' leave out the offsets it dropped.  With split, ranks other than 0
    get 'offsets' too (their own), as from run_destriper.
    residuals / residual_cut: as run_destriper's, every band's table from one device pass and the
    cut decided per band; each band's dict gains 'Residuals' (None on ranks other than 0).
    prior: not supported (NotImplementedError): the noise prior solves one band.
    solve_mask: as run_destriper's, one mask for all bands (the two-pass 'snr' form is per band:
    NotImplementedError here); each band's dict gains 'solve_mask' with that band's counts."""
    _mask_check(solve_mask, None, residual_cut)
    if _snr_spec(solve_mask) is not None:
        raise NotImplementedError("solve_mask ('snr', ...) is built per band: call run_destriper per band")
    if prior is not None:
        raise NotImplementedError('the noise prior solves one band: batched bands are not supported')
    import torch
    if device is None:
        device = torch.cuda.current_device()
    npix = int(pixel_edges[-1]) + 1
    tods = np.asarray(_tods, dtype=np.float64)
    if tods.ndim != 2:
        raise ValueError('_tods must be [n_bands, N]')
    resid = _residual_args(residuals, residual_cut, False, feedid, obsids)
    specs = split_specs(split, feedid, obsids, offset_length)
    dd = DeviceDestriper(np.asarray(_pointing), tods, np.asarray(_weights, dtype=np.float64), int(offset_length), npix,
                         device, keep=None if keep is None else np.asarray(keep, dtype=np.uint8), map_shape=map_shape,
                         split=None if specs is None else [(lab, len(names)) for lab, names in specs],
                         solve_mask=solve_mask, **resid)
    res = dd.solve(threshold, niter, to_host=True)
    d = _dist()
    rank = d.get_rank() if d is not None else 0
    out = []
    hm = res['maps']
    for b in range(tods.shape[0]):
        extra = {} if specs is None else _split_entries(specs, res['splits'], band=b)
        if solve_mask is not None:
            sm = res['solve_mask']
            extra['solve_mask'] = {'pixels': sm['pixels'], 'samples': int(sm['samples'][b]),
                                   'empty_offsets': int(sm['empty_offsets'][b]), 'mask': dd.mask_flags}
        if resid:
            extra['Residuals'] = _residual_table(dd, res['residuals'], band=b)
        if rank != 0:
            if specs is not None:        # every rank keeps the offsets its split sums were binned with
                extra['offsets'] = res['x'][b].cpu().numpy()
            out.append({'All': {'map': None, 'naive': None, 'weight': None, 'map2': None}, **extra})
            continue
        maps = {k: v[b] for k, v in hm.items()}
        out.append({'All': maps, 'iters': res['iters'][b], 'offsets': res['x'][b].cpu().numpy(), **extra})
    return out


# ---------------------------------------------------------------- bench helper
def car_pixels(ra, dec, nx=480, ny=480, cdelt=1.0 / 60.0, ra0=None, dec0=None):
    """Plate-carree pixel index (floor(x + 0.5) convention of transform_to_1d,
    COMAPData.py:83-117) of (ra, dec) on an nx x ny grid centred on (ra0, dec0);
    off-map -> -1.  A fp64 restatement of CAR without wcslib (WCS parity is
    SURVEY §8f row 1)."""
    import torch
    ra0 = float(torch.median(ra)) if ra0 is None else ra0
    dec0 = float(torch.median(dec)) if dec0 is None else dec0
    px = torch.floor(-(ra - ra0) / cdelt + (nx / 2 - 1) + 0.5)
    py = torch.floor((dec - dec0) / cdelt + (ny / 2 - 1) + 0.5)
    ok = (px >= 0) & (px <= nx - 1) & (py >= 0) & (py <= ny - 1)
    return torch.where(ok, py * nx + px, torch.full_like(px, -1)).to(torch.int32)


def level2_to_destriper_inputs(level2, data, band=0, offset_length=50):
    """Flat (tod, weights, pixels) device tensors from a Level-2 result: per
    feed and scan the first floor(n/L)*L samples (countDataSize,
    COMAPData.py:163-187), weights = averaged_tod/weights.  The cuts and the
    w=400 median filter of get_tod are SURVEY §8f row 1 (not applied here)."""
    import torch
    tod = level2['averaged_tod/tod']
    w = level2['averaged_tod/weights']
    dev = tod.device
    ra = torch.as_tensor(np.asarray(data['spectrometer/pixel_pointing/pixel_ra']), device=dev)
    dec = torch.as_tensor(np.asarray(data['spectrometer/pixel_pointing/pixel_dec']), device=dev)
    edges = np.asarray(level2['averaged_tod/scan_edges'])
    segs_t, segs_w, segs_p = [], [], []
    ra0, dec0 = float(torch.median(ra)), float(torch.median(dec))
    for f in range(tod.shape[0]):
        for s, e in edges:
            n = int((e - s) // offset_length * offset_length)
            if n <= 0:
                continue
            segs_t.append(tod[f, band, s:s + n])
            segs_w.append(w[f, band, s:s + n])
            segs_p.append(car_pixels(ra[f, s:s + n], dec[f, s:s + n], ra0=ra0, dec0=dec0))
    t = torch.cat(segs_t)
    ww = torch.cat(segs_w)
    pp = torch.cat(segs_p)
    bad = ~torch.isfinite(t)
    t = torch.where(bad, torch.zeros_like(t), t)
    ww = torch.where(bad | ~torch.isfinite(ww), torch.zeros_like(ww), ww)
    return t, ww, pp
