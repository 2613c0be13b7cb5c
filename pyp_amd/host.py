"""Host-side objects over the C ABI: Reference (prepared 3-D reference), refine(), Accumulator
(half-map accumulators + finalise).  Mirrors what the refine3d / reconstruct3d / merge3d processes
do between reading their inputs and writing their outputs."""
import ctypes as C

import numpy as np

from . import lib
from .abi import NCOL, STATS_COLS, K_NAMES, CreateMaskCfg, CreateMaskInfo, FinalCfg, FrameCfg, FrameInfo, LocresCfg, LocresInfo, MaskCfg, PostCfg, PostInfo, ReconCfg, RefineCfg  # noqa: F401


def _sync_producer(t):
    """The library works on its own HIP stream (include/ppm.h, "Stream ordering"): whatever torch has queued on the
    tensor's device (the copy or kernel that produced or zeroed it) must have finished before the raw pointer goes in."""
    import torch
    torch.cuda.current_stream(t.device).synchronize()


def _images_arg(images, n_img, box):
    """numpy array (host) or an object with data_ptr() on the GPU (torch tensor) -> (pointer, on_device, keepalive)."""
    if hasattr(images, "data_ptr") and hasattr(images, "is_cuda"):
        if not images.is_cuda:
            images = images.numpy()
        else:
            if not getattr(images, "ready", False):      # a torch tensor: wait for whatever torch queued on it (cli.DeviceImages arrives finished)
                _sync_producer(images)
            if str(images.dtype) != "torch.float32" or not images.is_contiguous():
                raise ValueError("ERROR: device image stack must be contiguous float32")
            if images.numel() != n_img * box * box:
                raise ValueError("ERROR: image stack size does not match the rows")
            return C.c_void_p(images.data_ptr()), 1, images
    a = np.ascontiguousarray(images, dtype=np.float32)
    if a.size != n_img * box * box:
        raise ValueError("ERROR: image stack size does not match the rows")
    return lib.ptr(a), 0, a


def _volumes_arg(volumes, n_vol, box):
    """numpy array (host) or a device array (torch tensor / anything with data_ptr(), is_cuda) -> (pointer, on_device, keepalive)."""
    if hasattr(volumes, "is_cuda") and volumes.is_cuda:
        if str(volumes.dtype) != "torch.float32" or not volumes.is_contiguous() or volumes.numel() != n_vol * box ** 3:
            raise ValueError("ERROR: device volumes must be contiguous float32 of V * box^3 elements")
        if not getattr(volumes, "ready", False):
            _sync_producer(volumes)
        return C.c_void_p(volumes.data_ptr()), 1, volumes
    a = np.ascontiguousarray(volumes.numpy() if hasattr(volumes, "numpy") else volumes, dtype=np.float32)
    if a.size != n_vol * box ** 3:
        raise ValueError("ERROR: volumes do not match the poses")
    return lib.ptr(a), 0, a


class Reference:
    """3-D reference prepared for projection matching up to `max_band_px` Fourier pixels."""

    def __init__(self, vol, max_band_px=None, device=0, pad=1, ring_weight=None):
        lib.init(device)
        vol = np.ascontiguousarray(vol, dtype=np.float32)
        if vol.ndim != 3 or len(set(vol.shape)) != 1:
            raise ValueError("ERROR: reference must be a cubic volume")
        self.n = vol.shape[0]
        band = self.n / 2 if max_band_px is None else float(max_band_px)
        w = None if ring_weight is None else np.ascontiguousarray(ring_weight, dtype=np.float32)
        self.h = lib.load().ppm_reference_create_weighted(lib.ptr(vol), self.n, band, int(pad), None if w is None else lib.ptr(w),
                                                          0 if w is None else int(w.size))
        if not self.h:
            raise lib.PpmError(lib.last_error())

    def refine(self, cfg, images, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != NCOL:
            raise ValueError("ERROR: rows must be (M, 32)")
        out = np.empty_like(rows)
        p, on_dev, keep = _images_arg(images, len(rows), cfg.box)
        lib.check(lib.load().ppm_refine_batch(self.h, C.byref(cfg), p, on_dev, len(rows), lib.ptr(rows), lib.ptr(out)))
        del keep
        return out

    def match_projections(self, cfg, rows):
        """Matching projections of refine3d (ppm_match_projections): float32 [M, box, box], the noise-free model of each row's particle."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != NCOL:
            raise ValueError("ERROR: rows must be (M, 32)")
        out = np.empty((len(rows), cfg.box, cfg.box), dtype=np.float32)
        lib.check(lib.load().ppm_match_projections(self.h, C.byref(cfg), lib.ptr(rows), len(rows), lib.ptr(out)))
        return out

    def csp_refine(self, cfg, csp_cfg, images, rows, particles, tilts):
        """Constrained refinement (ppm_csp_refine): returns updated copies (rows, particles, tilts)."""
        rows = np.array(rows, dtype=np.float64, order="C")
        particles = np.array(particles, dtype=np.float64, order="C")
        tilts = np.array(tilts, dtype=np.float64, order="C")
        if rows.ndim != 2 or rows.shape[1] != NCOL or particles.ndim != 2 or particles.shape[1] != 12 or tilts.ndim != 2 or tilts.shape[1] != 6:
            raise ValueError("ERROR: rows must be (M, 32), particles (P, 12), tilts (T, 6)")
        p, on_dev, keep = _images_arg(images, len(rows), cfg.box)
        lib.check(lib.load().ppm_csp_refine(self.h, C.byref(cfg), C.byref(csp_cfg), p, on_dev, len(rows), lib.ptr(rows), lib.ptr(particles),
                                            len(particles), lib.ptr(tilts), len(tilts)))
        del keep
        return rows, particles, tilts

    def frame_refine(self, cfg, fcfg, images, rows, maps=False):
        """Movie-frame refinement (ppm_frame_refine): one shift per frame row from score maps pooled over the neighbouring frames of its
        (PIND, TIND) group.  Returns (rows_out, info dict), with maps=True (rows_out, info, own_maps, pooled_maps), both (M, 2W + 1, 2W + 1)
        float32, row-major (jy, jx), zeros for rows without a map."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != NCOL:
            raise ValueError("ERROR: rows must be (M, 32)")
        L = lib.load()
        nst = C.c_int()
        lib.check(L.ppm_frame_plan(C.byref(fcfg), None, C.byref(nst), None))
        side = 2 * nst.value + 1
        out = np.empty_like(rows)
        info = FrameInfo()
        own = np.zeros((len(rows), side, side), dtype=np.float32) if maps else None
        pooled = np.zeros((len(rows), side, side), dtype=np.float32) if maps else None
        p, on_dev, keep = _images_arg(images, len(rows), cfg.box)
        lib.check(L.ppm_frame_refine(self.h, C.byref(cfg), C.byref(fcfg), p, on_dev, lib.ptr(rows), len(rows), lib.ptr(out),
                                     lib.ptr(own) if maps else None, lib.ptr(pooled) if maps else None, C.byref(info)))
        del keep
        return (out, info.as_dict(), own, pooled) if maps else (out, info.as_dict())

    def sva_align(self, cfg, volumes, wedges, poses, accumulator=None, index=None):
        """Sub-tomogram alignment (ppm_sva_align): volumes (V, N, N, N) float32 (numpy or CUDA tensor), wedges (V, 2) tilt limits in
        degrees, poses (V, 12) = N row-major + shift.  Returns (refined poses, scores).  accumulator: an Accumulator of the same box -
        every chunk is added to the sub-tomogram average at its refined poses while it is in device memory (ppm_sva_align_average;
        half-map = parity of index, default 0 .. V-1)."""
        poses = np.array(poses, dtype=np.float64, order="C")
        if poses.ndim != 2 or poses.shape[1] != 12:
            raise ValueError("ERROR: poses must be (V, 12)")
        w = np.ascontiguousarray(wedges, dtype=np.float32).reshape(len(poses), 2)
        scores = np.zeros(len(poses), dtype=np.float64)
        p, on_dev, keep = _volumes_arg(volumes, len(poses), cfg.box)
        if accumulator is None:
            lib.check(lib.load().ppm_sva_align(self.h, C.byref(cfg), p, on_dev, len(poses), lib.ptr(w), lib.ptr(poses), lib.ptr(scores)))
        else:
            idx = None if index is None else np.ascontiguousarray(index, dtype=np.int64)
            if idx is not None and idx.shape != (len(poses),):
                raise ValueError("ERROR: index must be (V,)")
            if accumulator._ext is not None:
                _sync_producer(accumulator._ext)
            lib.check(lib.load().ppm_sva_align_average(self.h, accumulator.h, C.byref(cfg), p, on_dev, len(poses), lib.ptr(w), lib.ptr(poses), lib.ptr(scores),
                                                       None if idx is None else lib.ptr(idx)))
        del keep
        return poses, scores

    def note(self):
        """Remarks of the last refine() the caller should log ("" if none)."""
        return (lib.load().ppm_refine_note(self.h) or b"").decode(errors="replace")

    def last_counts(self):
        v = [C.c_long() for _ in range(4)]
        lib.check(lib.load().ppm_refine_last_counts(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("n_global", "n_local", "samples_global", "samples_local"), [x.value for x in v]))

    def last_sections(self):
        """Sections of the orientation grid the last refine()'s grid search ran in (ppm_refine_last_sections); 0: it had none."""
        return int(lib.load().ppm_refine_last_sections(self.h))

    def last_overlap(self):
        """Hit-stage blocks per compute unit beside the grid search in the last refine() (ppm_refine_last_overlap); 0: serial order."""
        return int(lib.load().ppm_refine_last_overlap(self.h))

    def last_reuse(self):
        """(neighbour lane-gathers, reused ones) of the full-band compass sweeps of the last refine() (ppm_refine_last_reuse);
        counted only under PPM_LOCAL_REUSE_COUNT=1, (0, 0) otherwise."""
        v = [C.c_long(), C.c_long()]
        lib.check(lib.load().ppm_refine_last_reuse(self.h, C.byref(v[0]), C.byref(v[1])))
        return v[0].value, v[1].value

    def close(self):
        if getattr(self, "h", None):
            lib.load().ppm_reference_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Accumulator:
    """The two half-map accumulators of a reconstruction ({re, im, weight} per Fourier voxel)."""

    def __init__(self, box, pixel_size, symmetry="C1", device=0, ext_tensor=None):
        lib.init(device)
        self.box, self.pixel = int(box), float(pixel_size)
        self.nfloats = int(lib.load().ppm_accum_floats(self.box))
        self._ext = ext_tensor
        ext = None
        if ext_tensor is not None:
            if ext_tensor.numel() != self.nfloats or not ext_tensor.is_cuda or not ext_tensor.is_contiguous():
                raise ValueError("ERROR: external accumulator tensor has the wrong size or is not on the GPU")
            ext = C.c_void_p(ext_tensor.data_ptr())
        self.h = lib.load().ppm_accum_create(self.box, self.pixel, symmetry.encode(), ext)
        if not self.h:
            raise lib.PpmError(lib.last_error())

    def insert(self, cfg, images, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        p, on_dev, keep = _images_arg(images, len(rows), self.box)
        if self._ext is not None:
            _sync_producer(self._ext)
        lib.check(lib.load().ppm_insert_batch(self.h, C.byref(cfg), p, on_dev, len(rows), lib.ptr(rows)))
        del keep

    def sva_insert(self, cfg, volumes, wedges, poses, index=None):
        """Sub-tomogram average (ppm_sva_insert): add aligned sub-volumes (V, N, N, N) float32 (numpy or CUDA tensor) with their wedges
        (V, 2) and poses (V, 12) to the half-map accumulators; index (V,) decides the half (parity), default 0 .. V-1."""
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        if poses.ndim != 2 or poses.shape[1] != 12:
            raise ValueError("ERROR: poses must be (V, 12)")
        w = np.ascontiguousarray(wedges, dtype=np.float32).reshape(len(poses), 2)
        idx = None if index is None else np.ascontiguousarray(index, dtype=np.int64)
        if idx is not None and idx.shape != (len(poses),):
            raise ValueError("ERROR: index must be (V,)")
        p, on_dev, keep = _volumes_arg(volumes, len(poses), self.box)
        if self._ext is not None:
            _sync_producer(self._ext)
        lib.check(lib.load().ppm_sva_insert(self.h, C.byref(cfg), p, on_dev, len(poses), lib.ptr(w), lib.ptr(poses), None if idx is None else lib.ptr(idx)))
        del keep

    def counts(self):
        return [int(lib.load().ppm_accum_count(self.h, 0)), int(lib.load().ppm_accum_count(self.h, 1))]

    def set_counts(self, c0, c1):
        lib.load().ppm_accum_set_count(self.h, 0, int(c0))
        lib.load().ppm_accum_set_count(self.h, 1, int(c1))

    def reduce(self, comm, root=-1):
        """Sum this rank's accumulator and particle counters over the communicator (ppm_accum_reduce: RCCL on the library's
        stream; root < 0 = all-reduce).  `comm` comes from `make_comm` (or is the caller's own ncclComm_t pointer)."""
        if self._ext is not None:
            _sync_producer(self._ext)
        lib.check(lib.load().ppm_accum_reduce(self.h, C.c_void_p(comm), int(root)))

    def download(self):
        a = np.empty(self.nfloats, dtype=np.float32)
        if self._ext is not None:
            _sync_producer(self._ext)
        lib.check(lib.load().ppm_accum_download(self.h, lib.ptr(a)))
        return a

    def add(self, host):
        a = np.ascontiguousarray(host, dtype=np.float32)
        if a.size != self.nfloats:
            raise ValueError("ERROR: dump has the wrong size for this box")
        if self._ext is not None:
            _sync_producer(self._ext)
        lib.check(lib.load().ppm_accum_add(self.h, lib.ptr(a)))

    def finalize(self, fcfg):
        n = self.box
        h1 = np.empty((n, n, n), dtype=np.float32)
        h2 = np.empty_like(h1)
        fl = np.empty_like(h1)
        stats = np.zeros((n // 2 - 1, STATS_COLS), dtype=np.float64)
        if self._ext is not None:
            _sync_producer(self._ext)
        lib.check(lib.load().ppm_finalize(self.h, C.byref(fcfg), lib.ptr(h1), lib.ptr(h2), lib.ptr(fl), lib.ptr(stats)))
        return h1, h2, fl, stats

    def close(self):
        if getattr(self, "h", None):
            lib.load().ppm_accum_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id():
    """128 opaque bytes (ncclUniqueId) made by ONE rank; hand them to the others by any means."""
    buf = (C.c_char * 128)()
    lib.check(lib.load().ppm_comm_unique_id(buf))
    return bytes(buf)


def make_comm(n_ranks, rank, unique_id, device=0):
    """An RCCL communicator over the ranks' GPUs (ppm_comm_create; collective: returns when all ranks have joined)."""
    lib.init(device)
    if len(unique_id) != 128:
        raise ValueError("ERROR: the communicator id must be 128 bytes")
    buf = (C.c_char * 128).from_buffer_copy(unique_id)
    h = lib.load().ppm_comm_create(int(n_ranks), int(rank), buf)
    if not h:
        raise lib.PpmError(lib.last_error())
    return h


def comm_count(comm):
    """Ranks of the communicator as RCCL itself reports them (ppm_comm_count = ncclCommCount)."""
    n = lib.load().ppm_comm_count(comm)
    if n < 0:
        raise lib.PpmError(lib.last_error())
    return int(n)


def destroy_comm(comm):
    if comm:
        lib.load().ppm_comm_destroy(C.c_void_p(comm))


def extract_boxes(micrograph, coords, box, radius_A, pixel_size, coordinate_binning=1, normalize=True, fix_empty=True,
                  out=None, device=0):
    """Crop + normalise particle boxes (src/pyp/extract/core.py:447-506 with src/pyp/analysis/image.py:406-417).
    micrograph: 2-D float32 numpy array or CUDA tensor; coords: (M, 2) of (box[0], box[1]) = (column, row) coordinates;
    out: optional CUDA tensor (M, box, box) to fill in place (resident stack).  Returns the stack.  The rules are DESIGN.md section 8a;
    coordinates that are not finite or do not fit an int with the box to spare, and a negative or NaN radius, raise PpmError."""
    lib.init(device)
    coords = np.ascontiguousarray(coords, dtype=np.float64).reshape(-1, 2)
    m = len(coords)
    radius_px = float(radius_A) / (float(pixel_size) * float(coordinate_binning))
    if hasattr(micrograph, "is_cuda") and micrograph.is_cuda:
        if str(micrograph.dtype) != "torch.float32" or not micrograph.is_contiguous() or micrograph.dim() != 2:
            raise ValueError("ERROR: device micrograph must be a contiguous 2-D float32 tensor")
        _sync_producer(micrograph)
        ip, idev, rows, cols, keep = C.c_void_p(micrograph.data_ptr()), 1, micrograph.shape[0], micrograph.shape[1], micrograph
    else:
        a = np.ascontiguousarray(micrograph, dtype=np.float32)
        if a.ndim != 2:
            raise ValueError("ERROR: micrograph must be 2-D")
        ip, idev, rows, cols, keep = lib.ptr(a), 0, a.shape[0], a.shape[1], a
    if out is not None:
        if not out.is_cuda or out.numel() != m * box * box or not out.is_contiguous():
            raise ValueError("ERROR: output stack tensor has the wrong size or is not on the GPU")
        _sync_producer(out)
        op, odev, res = C.c_void_p(out.data_ptr()), 1, out
    else:
        res = np.empty((m, box, box), dtype=np.float32)
        op, odev = lib.ptr(res), 0
    lib.check(lib.load().ppm_extract_boxes(ip, idev, int(rows), int(cols), lib.ptr(coords), m, int(box), float(coordinate_binning),
                                           radius_px, int(bool(normalize)), int(bool(fix_empty)), op, odev))
    del keep
    return res


def _cubes(who, maps, out=None, out_box=None):
    """Shared front of the map entry points: `maps` = the maps of a call to `who`, N^3 float32 of one shape, all numpy arrays or all CUDA
    torch tensors; `out` = the caller's own array for the result (of the same kind; a cube of out_box, default N) or None.  Returns
    (on_device, N, maps, pointers, keep-alive); host maps come back as contiguous float32 arrays."""
    on_dev = bool(getattr(maps[0], "is_cuda", False))
    if any(bool(getattr(m, "is_cuda", False)) != on_dev for m in list(maps) + ([out] if out is not None else [])):
        raise ValueError(f"ERROR: {who}: the maps and out must all be on the host or all on the device")
    if not on_dev:
        maps = [np.ascontiguousarray(m.numpy() if hasattr(m, "numpy") else m, dtype=np.float32) for m in maps]
    shape = tuple(int(x) for x in maps[0].shape)
    if len(shape) != 3 or len(set(shape)) != 1:
        raise ValueError(f"ERROR: {who}: the maps must be cubic volumes")
    if any(tuple(int(x) for x in m.shape) != shape for m in maps):
        raise ValueError(f"ERROR: {who}: the maps have different dimensions")
    n = shape[0]
    if out is not None:
        oshape = (n if out_box is None else int(out_box),) * 3
        if on_dev and tuple(out.shape) != oshape:
            raise ValueError(f"ERROR: {who}: out has the wrong shape")
        if not on_dev and (not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.shape != oshape or not out.flags.c_contiguous):
            raise ValueError(f"ERROR: {who}: out must be a contiguous float32 array of shape {oshape}")
    if on_dev:
        keep = [_volumes_arg(m, 1, n) for m in maps]
        return True, n, list(maps), [k[0] for k in keep], keep
    return False, n, maps, [lib.ptr(m) for m in maps], maps


def _cube_out(like, on_dev, box, out=None):
    """(result, pointer): `out` where the caller gave one (checked by _cubes), else a new box^3 float32 array of the kind of `like`."""
    if on_dev:
        import torch
        res = torch.empty((box,) * 3, dtype=torch.float32, device=like.device) if out is None else out
        return res, _volumes_arg(res, 1, box)[0]
    res = np.empty((box,) * 3, dtype=np.float32) if out is None else out
    return res, lib.ptr(res)


def mask_volume(vol, mask, cfg, out=None, device=0):
    """Shape-mask a map (ppm_mask_volume, what apply_mask.exe does to last iteration's map): vol, mask = N^3 float32, both numpy
    arrays or both CUDA torch tensors; cfg: abi.MaskCfg.  Returns an array of the kind it was given; `out` (same kind and shape, may
    be `vol` itself) receives the result in place of a new array."""
    lib.init(device)
    on_dev, n, maps, (pv, pm), keep = _cubes("mask_volume", [vol, mask], out)
    res, po = _cube_out(maps[0], on_dev, n, out)
    lib.check(lib.load().ppm_mask_volume(pv, pm, 1 if on_dev else 0, n, C.byref(cfg), po))
    del keep
    return res


def create_mask(vol, cfg, out=None, device=0):
    """Binary mask of a map's largest body (ppm_create_mask, what frealignx/create_mask does in PYP's masking block): vol = N^3
    float32, a numpy array or a CUDA torch tensor; cfg: abi.CreateMaskCfg.  Returns (mask, info): the mask is of the kind of `vol`
    (`out`, same kind and shape, receives it in place of a new array), info an abi.CreateMaskInfo.  A refusal - a threshold no voxel
    reaches among them - raises lib.PpmError and leaves `out` as it was."""
    lib.init(device)
    on_dev, n, maps, (pv,), keep = _cubes("create_mask", [vol], out)
    res, po = _cube_out(maps[0], on_dev, n, out)
    info = CreateMaskInfo()
    lib.check(lib.load().ppm_create_mask(pv, 1 if on_dev else 0, n, C.byref(cfg), po, C.byref(info)))
    del keep
    return res, info


def postprocess(half1, half2, cfg, mask=None, device=0):
    """Post-processing of two half maps (ppm_postprocess, what PYP's external/postprocessing/postprocessing.py does): half1, half2 and
    the optional external mask = N^3 float32, all numpy arrays or all CUDA torch tensors; cfg: abi.PostCfg (mask given: cfg.mask_mode
    must be "external").  Returns dict(unmasked, masked, mask = maps of the kind given; curves = [4, N/2 + 1] float64 (unmasked,
    masked, phase-randomised, corrected FSC); shell_count = [N/2 + 1] int64; info = abi.PostInfo).  A refusal raises lib.PpmError."""
    lib.init(device)
    on_dev, n, maps, ptrs, keep = _cubes("postprocess", [half1, half2] + ([mask] if mask is not None else []))
    outs, po = zip(*[_cube_out(maps[0], on_dev, n) for _ in range(3)])
    ns = n // 2 + 1
    curves, counts, info = np.zeros((4, ns), dtype=np.float64), np.zeros(ns, dtype=np.int64), PostInfo()
    lib.check(lib.load().ppm_postprocess(ptrs[0], ptrs[1], ptrs[2] if mask is not None else None, 1 if on_dev else 0, n, C.byref(cfg),
                                         po[0], po[1], po[2], lib.ptr(curves), lib.ptr(counts), C.byref(info)))
    del keep
    return dict(unmasked=outs[0], masked=outs[1], mask=outs[2], curves=curves, shell_count=counts, info=info)


def local_resolution(half1, half2, cfg, mask=None, device=0):
    """Local resolution of two half maps (ppm_local_resolution, what ResMap --noguiSplit does in PYP's Post-processing block; DESIGN.md
    2e): half1, half2 and the optional mask (inside where > 0.5; default: the sphere of radius N/2) = N^3 float32, all numpy arrays or all
    CUDA torch tensors; cfg: abi.LocresCfg.  Returns dict(resolution = map of the kind given, in A, 100 where nothing was assigned;
    levels, tau = [L] float32; counts = [L] int64, voxels per level; info = abi.LocresInfo), and with cfg.keep_levels also energies =
    [L, N, N, N, 2] float32 of the kind given: E_A and E_D of every level.  A refusal raises lib.PpmError."""
    from . import abi
    lib.init(device)
    on_dev, n, maps, ptrs, keep = _cubes("local_resolution", [half1, half2] + ([mask] if mask is not None else []))
    call = LocresCfg(pixel_size=cfg.pixel_size, p_value=cfg.p_value, min_res=cfg.min_res, max_res=cfg.max_res, step=cfg.step, keep_levels=0)
    energies, pe = None, None
    if cfg.keep_levels:
        try:
            call.keep_levels = len(abi.locres_levels(n, cfg.pixel_size, cfg.min_res, cfg.max_res, cfg.step)[0])
        except ValueError as e:
            raise lib.PpmError(str(e))
        if on_dev:
            import torch
            energies = torch.empty((call.keep_levels, n, n, n, 2), dtype=torch.float32, device=maps[0].device)
            pe = C.c_void_p(energies.data_ptr())
        else:
            energies = np.empty((call.keep_levels, n, n, n, 2), dtype=np.float32)
            pe = lib.ptr(energies)
    out, po = _cube_out(maps[0], on_dev, n)
    info = LocresInfo()
    lib.check(lib.load().ppm_local_resolution(C.byref(call), ptrs[0], ptrs[1], ptrs[2] if mask is not None else None, 1 if on_dev else 0, n,
                                              po, pe, C.byref(info)))
    del keep
    L = info.n_levels
    res = dict(resolution=out, levels=np.array(info.levels[:L], dtype=np.float32), tau=np.array(info.tau[:L], dtype=np.float32),
               counts=np.array(info.counts[:L], dtype=np.int64), info=info)
    if energies is not None:
        res["energies"] = energies
    return res


def _items_in_out(x, n_out, volume, out, who):
    """Shared front of resample() / resize(): x = one image [N, N], a stack [n, N, N] or, with volume=True, a volume [N, N, N]; numpy array
    or CUDA torch tensor.  Returns (x, result, dims, n_items, n_in, pointer in, pointer out, on_device)."""
    on_dev = bool(getattr(x, "is_cuda", False))
    if out is not None and on_dev != bool(getattr(out, "is_cuda", False)):
        raise ValueError(f"ERROR: {who}: input and out must both be on the host or both on the device")
    if not on_dev:
        x = np.ascontiguousarray(x.numpy() if hasattr(x, "numpy") else x, dtype=np.float32)
    shape = tuple(int(s) for s in x.shape)
    if len(shape) == 2 and not volume:
        dims, n_items = 2, 1
    elif len(shape) == 3:
        dims, n_items = (3, 1) if volume else (2, shape[0])
    else:
        raise ValueError(f"ERROR: {who}: expected an image, a stack of images or (volume=True) a volume, got shape {shape}")
    n_in, n_out = shape[-1], int(n_out)
    if len(set(shape[-dims:])) != 1:
        raise ValueError(f"ERROR: {who}: only square images and cubic volumes are supported, got shape {shape}")
    if n_items < 1:
        raise ValueError(f"ERROR: {who}: the stack is empty")
    oshape = shape[:len(shape) - dims] + (n_out,) * dims
    if on_dev:
        import torch
        if str(x.dtype) != "torch.float32" or not x.is_contiguous():
            raise ValueError(f"ERROR: {who}: a device array must be contiguous float32")
        res = torch.empty(oshape, dtype=torch.float32, device=x.device) if out is None else out
        if tuple(res.shape) != oshape or str(res.dtype) != "torch.float32" or not res.is_contiguous():
            raise ValueError(f"ERROR: {who}: out must be a contiguous float32 tensor of shape {oshape}")
        for t in (x, res):
            if not getattr(t, "ready", False):
                _sync_producer(t)
        pi, po = C.c_void_p(x.data_ptr()), C.c_void_p(res.data_ptr())
    else:
        res = np.empty(oshape, dtype=np.float32) if out is None else out
        if not isinstance(res, np.ndarray) or res.dtype != np.float32 or res.shape != oshape or not res.flags.c_contiguous:
            raise ValueError(f"ERROR: {who}: out must be a contiguous float32 array of shape {oshape}")
        pi, po = lib.ptr(x), lib.ptr(res)
    return x, res, dims, n_items, n_in, pi, po, on_dev


def resample(x, n_out, volume=False, out=None, device=0):
    """Fourier resampling (ppm_resample; what cistem2's resample and frealign_v9.11's resample_mp.exe do): every image of a
    stack [n, N, N] (or one image [N, N]) to n_out x n_out, or with volume=True a volume [N, N, N] to n_out^3.  numpy array or CUDA torch
    tensor in, the same kind out (`out`, same kind, receives it in place of a new array).  Both sizes must be ones the transforms take; a
    refusal raises lib.PpmError and leaves `out` as it was."""
    lib.init(device)
    x, res, dims, n_items, n_in, pi, po, on_dev = _items_in_out(x, n_out, volume, out, "resample")
    lib.check(lib.load().ppm_resample(pi, 1 if on_dev else 0, dims, n_items, n_in, int(n_out), po))
    return res


def resize(x, n_out, normalize=False, volume=False, out=None, device=0, pad_values=False):
    """Crop or pad about the centre (ppm_resize; what cistem2's resize does): the pad value is the mean of the faces of a
    volume / of the four edges of every image; normalize: mean 0, standard deviation 1 first.  Arguments as for resample(); sizes 8..512.
    pad_values=True: returns (result, float32 array of the pad value of every item)."""
    lib.init(device)
    x, res, dims, n_items, n_in, pi, po, on_dev = _items_in_out(x, n_out, volume, out, "resize")
    pads = np.zeros(n_items, dtype=np.float32)
    lib.check(lib.load().ppm_resize(pi, 1 if on_dev else 0, dims, n_items, n_in, int(n_out), 1 if normalize else 0, po, lib.ptr(pads)))
    return (res, pads) if pad_values else res


def fit_plan(n_in, pixel_in, pixel_out, box):
    """The plan of fit_reference (ppm_fit_plan; no device needed): abi.FitInfo.  A pair of sizes more than 1 % off raises lib.PpmError
    whose text names the best achievable pixel size."""
    from .abi import FitInfo
    info = FitInfo()
    lib.check(lib.load().ppm_fit_plan(int(n_in), float(pixel_in), float(pixel_out), int(box), C.byref(info)))
    return info


def fit_reference(vol, pixel_in, pixel_out, box, out=None, device=0):
    """Bring a reference map to the data's box and pixel size (ppm_fit_volume): resize to P, resample P -> M, resize to
    `box`.  vol: cubic float32, numpy array or CUDA torch tensor.  Returns (map of the kind given, abi.FitInfo); info.pixel_achieved is the
    pixel size the map really has (within 1 % of pixel_out)."""
    from .abi import FitInfo
    lib.init(device)
    box = int(box)
    on_dev, n, maps, (pv,), keep = _cubes("fit_reference", [vol], out, out_box=box)
    res, po = _cube_out(maps[0], on_dev, box, out)
    info = FitInfo()
    lib.check(lib.load().ppm_fit_volume(pv, 1 if on_dev else 0, n, float(pixel_in), float(pixel_out), box, po, C.byref(info)))
    del keep
    return res, info


def periodogram_plan(shape, tile, group=1):
    """The plan of periodogram() (ppm_ctf_spectrum_plan; no device needed): abi.CtfSpectrumInfo.  shape: (ny, nx) of an image or
    (nframes, ny, nx) of a movie.  A refusal raises lib.PpmError."""
    from .abi import CtfSpectrumInfo
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"ERROR: periodogram: expected an image [ny, nx] or a movie [nframes, ny, nx], got shape {shape}")
    nf, ny, nx = ((1,) + shape)[-3:]
    info = CtfSpectrumInfo()
    lib.check(lib.load().ppm_ctf_spectrum_plan(nx, ny, nf, int(group), int(tile), C.byref(info)))
    return info


class CtfEstimator:
    """Handle of the CTF estimation stages (ppm_ctf_create): owns their device workspaces, which are grown on demand, reused across
    calls and freed with the handle."""

    def __init__(self, device=0):
        lib.init(device)
        self.h = lib.load().ppm_ctf_create()
        if not self.h:
            raise lib.PpmError(lib.last_error())

    def periodogram(self, image, tile, normalise=True, group=1, out=None):
        """See host.periodogram."""
        on_dev = bool(getattr(image, "is_cuda", False))
        if not on_dev:
            image = np.ascontiguousarray(image.numpy() if hasattr(image, "numpy") else image, dtype=np.float32)
        elif str(image.dtype) != "torch.float32" or not image.is_contiguous():
            raise ValueError("ERROR: periodogram: a device image must be contiguous float32")
        info = periodogram_plan(image.shape, tile, group)
        nf, ny, nx = ((1,) + tuple(int(s) for s in image.shape))[-3:]
        oshape = (info.tile, info.half_w)
        if on_dev:
            import torch
            res = torch.empty(oshape, dtype=torch.float32, device=image.device) if out is None else out
            if tuple(res.shape) != oshape or str(res.dtype) != "torch.float32" or not res.is_contiguous() or not res.is_cuda:
                raise ValueError(f"ERROR: periodogram: out must be a contiguous float32 device tensor of shape {oshape}")
            for t in (image, res):
                if not getattr(t, "ready", False):
                    _sync_producer(t)
            pi, po = C.c_void_p(image.data_ptr()), C.c_void_p(res.data_ptr())
        else:
            res = np.empty(oshape, dtype=np.float32) if out is None else out
            if not isinstance(res, np.ndarray) or res.dtype != np.float32 or res.shape != oshape or not res.flags.c_contiguous:
                raise ValueError(f"ERROR: periodogram: out must be a contiguous float32 array of shape {oshape}")
            pi, po = lib.ptr(image), lib.ptr(res)
        lib.check(lib.load().ppm_ctf_spectrum(self.h, pi, 1 if on_dev else 0, nx, ny, nf, int(group), int(tile), 1 if normalise else 0,
                                              po, 1 if on_dev else 0))
        return res

    def fit(self, spectra, cfg, windows=None, grid_scores=False, profile=False):
        """See host.estimate_ctf (the spectra form)."""
        on_dev = bool(getattr(spectra, "is_cuda", False))
        if not on_dev:
            spectra = np.ascontiguousarray(spectra.numpy() if hasattr(spectra, "numpy") else spectra, dtype=np.float32)
        elif str(spectra.dtype) != "torch.float32" or not spectra.is_contiguous():
            raise ValueError("ERROR: estimate_ctf: device spectra must be contiguous float32")
        shape = tuple(int(s) for s in spectra.shape)
        if len(shape) == 2:
            shape = (1,) + shape
        if len(shape) != 3 or shape[2] != shape[1] // 2 + 1:
            raise ValueError(f"ERROR: estimate_ctf: spectra must be [T, T / 2 + 1] or [n, T, T / 2 + 1], got shape {shape}")
        n, tile = shape[0], shape[1]
        info = fit_ctf_plan(tile, cfg)
        lo = hi = None
        ni_max = info.ni
        if windows is not None:
            w = np.ascontiguousarray(windows, dtype=np.float64).reshape(n, 2)
            lo, hi = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
            ni_max = int(np.floor((hi - lo) / cfg.step + 1e-9).max()) + 1 if (hi >= lo).all() else 1
        rows = np.zeros((n, 8), dtype=np.float64)
        scores = np.full((n, max(1, ni_max) * info.nc), np.nan, dtype=np.float32) if grid_scores else None
        if on_dev and not getattr(spectra, "ready", False):
            _sync_producer(spectra)
        ps = C.c_void_p(spectra.data_ptr()) if on_dev else lib.ptr(spectra)
        avrot = np.zeros((n, 6, info.B // 2 + 1), dtype=np.float64) if profile else None
        diag = np.zeros((n, info.B, info.B), dtype=np.float32) if profile else None
        lib.check(lib.load().ppm_ctf_fit(self.h, ps, 1 if on_dev else 0, n, tile, C.byref(cfg), None if lo is None else lib.ptr(lo),
                                         None if hi is None else lib.ptr(hi), lib.ptr(rows), None if scores is None else lib.ptr(scores),
                                         0 if scores is None else scores.shape[1], None if avrot is None else lib.ptr(avrot),
                                         None if diag is None else lib.ptr(diag)))
        out = (rows,) + ((scores,) if grid_scores else ()) + ((avrot, diag) if profile else ())
        return out if len(out) > 1 else rows

    def estimate(self, image, tile, cfg, group=1, profile=False):
        """See host.estimate_ctf (the image form)."""
        on_dev = bool(getattr(image, "is_cuda", False))
        if not on_dev:
            image = np.ascontiguousarray(image.numpy() if hasattr(image, "numpy") else image, dtype=np.float32)
        elif str(image.dtype) != "torch.float32" or not image.is_contiguous():
            raise ValueError("ERROR: estimate_ctf: a device image must be contiguous float32")
        periodogram_plan(image.shape, tile, group)
        nf, ny, nx = ((1,) + tuple(int(s) for s in image.shape))[-3:]
        if on_dev and not getattr(image, "ready", False):
            _sync_producer(image)
        row = np.zeros((1, 8), dtype=np.float64)
        info = fit_ctf_plan(tile, cfg)
        avrot = np.zeros((1, 6, info.B // 2 + 1), dtype=np.float64) if profile else None
        diag = np.zeros((1, info.B, info.B), dtype=np.float32) if profile else None
        lib.check(lib.load().ppm_ctf_estimate(self.h, C.c_void_p(image.data_ptr()) if on_dev else lib.ptr(image), 1 if on_dev else 0, nx, ny, nf,
                                              int(group), int(tile), C.byref(cfg), lib.ptr(row), None if avrot is None else lib.ptr(avrot),
                                              None if diag is None else lib.ptr(diag)))
        return (row, avrot, diag) if profile else row

    def close(self):
        if getattr(self, "h", None):
            lib.load().ppm_ctf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_ctf_estimators = {}


def periodogram(image, tile, normalise=True, group=1, out=None, device=0):
    """Averaged periodogram of a micrograph [ny, nx] or a movie [nframes, ny, nx] (ppm_ctf_spectrum; the spectrum stage of
    ctffind): |rfft2|^2 of tile x tile windows at stride tile / 2, the last row and column pulled back inside, averaged.  A movie's frames
    are averaged in groups of `group` first.  normalise=True applies the reference's own scaling ([0, 0] = 0, divide by the maximum);
    the result is then what its periodogram_averaging(image, tile, power=2) returns.  numpy array or CUDA torch tensor in, the same kind
    out, float32 [tile, tile // 2 + 1].  The tile must be a size the transforms take; a refusal raises lib.PpmError and leaves `out`
    as it was.  The workspaces belong to one CtfEstimator per device, kept for the life of the process."""
    return _ctf_estimator(device).periodogram(image, tile, normalise=normalise, group=group, out=out)


CTF_ROW = ("df1", "df2", "angle", "score", "grid_index", "grid_score", "samples", "fit_resolution")


def fit_ctf_plan(tile, cfg):
    """The plan of a fit (ppm_ctf_fit_plan; no device needed): abi.CtfFitInfo.  A refusal raises lib.PpmError."""
    from .abi import CtfFitInfo
    info = CtfFitInfo()
    lib.check(lib.load().ppm_ctf_fit_plan(int(tile), C.byref(cfg), C.byref(info)))
    return info


def _ctf_estimator(device):
    est = _ctf_estimators.get(device)
    if est is None:
        est = _ctf_estimators[device] = CtfEstimator(device)
    return est


def estimate_ctf(image_or_spectra, cfg, tile=None, group=1, windows=None, grid_scores=False, profile=False, device=0):
    """Defocus and astigmatism on the GPU (ppm_ctf_fit / ppm_ctf_estimate; the work of ctffind).  cfg: abi.CtfCfg.
    With tile=T the first argument is a micrograph [ny, nx] or a movie [nframes, ny, nx] (frames averaged in groups of `group`): its
    averaged periodogram is fitted without leaving the device.  With tile=None it is one spectrum [T, T / 2 + 1] or a batch
    [n, T, T / 2 + 1] as periodogram() returns them (numpy or CUDA tensor); windows [n, 2] then gives every spectrum its own
    [min_def, max_def].  Returns float64 rows [n, 8], columns host.CTF_ROW; with grid_scores=True also the float32 score map
    [n, candidates] of the grid search (NaN where a spectrum's window has fewer candidates); with profile=True also the six avrot rows
    float64 [n, 6, B / 2 + 1] (frequency in 1/A, rotational average, average along equiphase lines, fit, quality, noise level) and the
    diagnostic images float32 [n, B, B] (include/ppm.h)."""
    est = _ctf_estimator(device)
    if tile is not None:
        if windows is not None or grid_scores:
            raise ValueError("ERROR: estimate_ctf: windows and grid_scores go with spectra, not with an image")
        return est.estimate(image_or_spectra, tile, cfg, group=group, profile=profile)
    return est.fit(image_or_spectra, cfg, windows=windows, grid_scores=grid_scores, profile=profile)


def local_ctf(stack, weights, cfg, meandef, tolerance=500.0, device=0, return_spectra=False):
    """Per-particle defocus of one micrograph's particles (what the reference's ctffind_spr_local_estimate does with one process per
    particle): the one-tile periodogram of every particle of stack [P, B, B], mixed on the device as weights @ spectra with the caller's
    [P, P] weight matrix (the reference's distance weights), every mix fitted in one ppm_ctf_fit on meandef +- tolerance.  Returns the
    float64 table [P, 4] the reference writes to <name>_ctf.txt: df1, df2, angle, score; with return_spectra=True also the mixed spectra
    that were fitted (a CUDA tensor [P, B, B / 2 + 1])."""
    import torch
    est = _ctf_estimator(device)
    on_dev = bool(getattr(stack, "is_cuda", False))
    dev = stack.device if on_dev else torch.device("cuda", device)
    st = stack if on_dev else torch.from_numpy(np.ascontiguousarray(stack, dtype=np.float32)).to(dev)
    if st.dim() != 3 or st.shape[1] != st.shape[2]:
        raise ValueError(f"ERROR: local_ctf: expected a stack [P, B, B], got shape {tuple(st.shape)}")
    n, box = int(st.shape[0]), int(st.shape[1])
    w = torch.as_tensor(np.asarray(weights, dtype=np.float32) if not hasattr(weights, "is_cuda") else weights, dtype=torch.float32, device=dev)
    if tuple(w.shape) != (n, n):
        raise ValueError(f"ERROR: local_ctf: weights must be [{n}, {n}]")
    spectra = torch.empty((n, box, box // 2 + 1), dtype=torch.float32, device=dev)
    for i in range(n):
        est.periodogram(st[i], box, normalise=False, out=spectra[i])
    mixed = (w @ spectra.reshape(n, -1)).reshape(spectra.shape).contiguous()
    md = np.broadcast_to(np.asarray(meandef, dtype=np.float64), (n,))
    rows = est.fit(mixed, cfg, windows=np.stack([md - tolerance, md + tolerance], axis=1))
    table = np.ascontiguousarray(rows[:, :4])
    return (table, mixed) if return_spectra else table


class PinnedBuffer:
    """Page-locked host memory as a float32 numpy array (ppm_host_alloc): staging for uploads that overlap compute."""

    def __init__(self, n_floats, device=0, ptr=None):
        """ptr: memory already page-locked by ppm_host_alloc (surface/warm.py hands over what it prepared); owned from here on."""
        lib.init(device)
        self.n = int(n_floats)
        self.ptr = ptr or lib.load().ppm_host_alloc(self.n * 4)
        if not self.ptr:
            raise lib.PpmError(lib.last_error())
        self.array = np.ctypeslib.as_array((C.c_float * self.n).from_address(self.ptr))

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            lib.load().ppm_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def profile(enable=True, reset=True):
    lib.load().ppm_profile_enable(1 if enable else 0)
    if reset:
        lib.load().ppm_profile_reset()


def profile_report():
    out = {}
    for i, name in enumerate(K_NAMES):
        ms, n = C.c_double(), C.c_long()
        lib.check(lib.load().ppm_profile_get(i, C.byref(ms), C.byref(n)))
        out[name] = {"ms": ms.value, "launches": n.value}
    return out
