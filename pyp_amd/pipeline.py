"""One refinement iteration held in memory: refine -> select -> reconstruct -> finalise (the work of
`split_refinement` (frealign.py:3014-3193), `shape_phase_residuals` (scores.py:300-761), `split_reconstruction` (:1622-1835),
`local_merge_reconstruction` / `merge_reconstructions` (:1838-2175) for one class), without the files in between.
Sharded runs call this once per rank and reduce the accumulator with `pyp_amd.dist.reduce_accumulators`."""
import numpy as np

from . import host, select
from .abi import FinalCfg, MaskCfg, ReconCfg
from .formats.cistem import COL


def iteration(vol, stack, rows, refine_cfg, *, pixel_size, molecular_mass_kda, symmetry="C1", keep_fraction=1.0,
              score_weight_bfactor=0.0, outer_radius=None, split_by_pind=False, mask=None, mask_cfg=None, auto_mask=None, postprocess=None,
              local_resolution=None, reference_pixel=None):
    """vol: current reference (N^3 float32); stack: [M, N, N] float32 (numpy or a CUDA torch tensor); rows: [M, 32].
    mask (N^3 float32, of the same kind as vol) with mask_cfg (abi.MaskCfg; default: PYP's edge of 3 voxels, weight 0): the
    reference is shape-masked on the device first, as `shape_mask_reference` (align/core.py:783-856) does with apply_mask.exe.
    auto_mask (abi.CreateMaskCfg) in place of mask: the mask is made from vol itself on the device (host.create_mask, the work of
    `cistem_mask_create`, inout/image/core.py:1538-1605) and applied with mask_cfg.
    postprocess (abi.PostCfg): the half maps go through host.postprocess (the work of the Post-processing block, pyp_main.py:6601-6865)
    and its result is added as "post"; a cfg with mask "external" uses `mask` (or the one auto_mask made).
    local_resolution (abi.LocresCfg): the half maps go through host.local_resolution (the work of ResMap in the same block,
    pyp_main.py:6815-6844) and its result is added as "local_resolution"; `mask` (or the one auto_mask made), where there is one, says
    which voxels are inside.
    reference_pixel (A): vol may have any box and this pixel size; it is fitted to the stack's box and refine_cfg.pixel_size first
    (host.fit_reference, the work of `resize_initial_model`, preprocess/core.py:796-832); the plan is added as "fit".  A mask refers to
    the fitted map.
    Returns dict(rows=refined table incl. OCC after selection, half1, half2, filtered, stats=[N/2-1, 7] statistics table).
    """
    n = int(refine_cfg.box)
    if postprocess is not None and postprocess.mask_mode == 1 and mask is None and auto_mask is None:
        raise ValueError("ERROR: iteration: postprocess asks for an external mask, but neither mask nor auto_mask was given")
    fit_info = None
    if reference_pixel is not None:
        vol, fit_info = host.fit_reference(vol, reference_pixel, refine_cfg.pixel_size, n)
        if getattr(vol, "is_cuda", False) and mask is None and auto_mask is None:      # Reference takes a host array
            vol = vol.cpu().numpy()
    if auto_mask is not None:
        if mask is not None:
            raise ValueError("ERROR: iteration: auto_mask and mask exclude each other")
        mask, _ = host.create_mask(vol, auto_mask)
    post_mask = mask if postprocess is not None and postprocess.mask_mode == 1 else None
    locres_mask = mask if local_resolution is not None else None
    if mask is not None:
        vol = host.mask_volume(vol, mask, mask_cfg if mask_cfg is not None else MaskCfg.make(pixel_size=pixel_size))
        if getattr(vol, "is_cuda", False):          # map and mask were device tensors: Reference takes a host array
            vol = vol.cpu().numpy()
    elif mask_cfg is not None:
        raise ValueError("ERROR: iteration: mask_cfg given without a mask")
    ref = host.Reference(vol, n / 2)
    try:
        refined = ref.refine(refine_cfg, stack, rows)
    finally:
        ref.close()
    used = select.select_particles(refined, threshold=keep_fraction) if keep_fraction < 1.0 else refined
    score = used[used[:, COL["OCCUPANCY"]] > 0, COL["SCORE"]]
    rc = ReconCfg(box=n, pixel_size=pixel_size, res_limit=2 * pixel_size, score_weight_bfactor=score_weight_bfactor,
                  score_average=float(score.mean()) if score.size else 0.0, score_threshold=0.0, normalize=1, invert=0,
                  split_by_pind=1 if split_by_pind else 0, mask_radius=refine_cfg.mask_radius)
    acc = host.Accumulator(n, pixel_size, symmetry)
    try:
        acc.insert(rc, stack, used)
        fc = FinalCfg(molecular_mass_kda=molecular_mass_kda, inner_radius=0.0,
                      outer_radius=outer_radius if outer_radius is not None else 0.45 * n * pixel_size, mask_falloff=0.0)
        h1, h2, filt, stats = acc.finalize(fc)
    finally:
        acc.close()
    result = dict(rows=used, half1=h1, half2=h2, filtered=filt, stats=np.asarray(stats))
    if fit_info is not None:
        result["fit"] = fit_info
    if postprocess is not None:
        if getattr(post_mask, "is_cuda", False):      # the half maps are host arrays
            post_mask = post_mask.cpu().numpy()
        result["post"] = host.postprocess(h1, h2, postprocess, mask=post_mask)
    if local_resolution is not None:
        if getattr(locres_mask, "is_cuda", False):
            locres_mask = locres_mask.cpu().numpy()
        result["local_resolution"] = host.local_resolution(h1, h2, local_resolution, mask=locres_mask)
    return result
