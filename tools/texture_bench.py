#!/usr/bin/env python
"""Times the texture bake at full size: the bench template (build_synthetic_scene + discretizeSDF), synthetic.per_face_atlas UVs,
540 x 540 views, R = 1680, K = 120, the reference's defaults.  Per kernel: HIP-event time (median of --reps after a warm-up of at least
--warmup-seconds, so the clock has settled), the bytes the kernel has to move, the achieved GB/s, and a plain device copy of the same
byte count timed in the same process.  Prints a markdown table (profiles/texture_bake.md is one run of it) and one JSON line.

There is nothing to compare against: the reference's texture_mesh_extract.py needs opendr / VideoAvatar / cv2 and cannot run here, and
the parent commit has no texture stage.  No speed-up is claimed.

    python tools/texture_bench.py [--views 120] [--resolution 1680] [--reps 20] [--out profiles/texture_bake.md]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def _copy_ms(nbytes, reps):
    """a device copy that moves `nbytes` in total (half read, half written)"""
    n = max(int(nbytes) // 2, 1 << 12)
    src = torch.empty(n, dtype=torch.uint8, device="cuda:0"); dst = torch.empty_like(src)
    return _timed(lambda: dst.copy_(src), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=120)
    ap.add_argument("--resolution", type=int, default=1680)
    ap.add_argument("--image", type=int, default=540)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup-seconds", type=float, default=3.0)
    ap.add_argument("--batch", type=int, default=8, help="views per set of launches while the view terms are prepared")
    ap.add_argument("--out", default=None, help="also write the markdown table here")
    args = ap.parse_args()
    from selfreconcode_amd.ops import rasterize_meshes, vertex_adjacency, vertex_normals
    from selfreconcode_amd.synthetic import build_synthetic_scene, per_face_atlas
    from selfreconcode_amd.posed import FULL_RATIO
    from selfreconcode_amd.texture import bake_texture, texture_frames
    from selfreconcode_amd.texture_ops import TextureAccumulator, face_visibility, fill, uv_texel_map, view_alpha
    dev = "cuda:0"
    K, R, H = args.views, args.resolution, args.image
    net, ds, _ = build_synthetic_scene(device=dev, frame_num=max(2 * K, 64), H=H, W=H, consistent_masks=False, opt_camera=False)
    with torch.no_grad():
        verts, faces = net.discretizeSDF(FULL_RATIO, None, 0.0)
    verts, faces = verts.detach(), faces[(faces >= 0).all(1)].long().contiguous()
    V, F = verts.shape[0], faces.shape[0]
    vt, ft = per_face_atlas(F, R, 0.5)
    vt, ft = vt.to(dev), ft.to(dev)
    fids = torch.as_tensor(texture_frames(ds.frame_num, K), device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev).float(), torch.arange(H, device=dev).float(), indexing="ij")
    images = torch.stack([0.5 + 0.4 * torch.sin(xs / (40. + c) + ys / (55. + 2 * c) + 0.1 * c) for c in range(3)], -1)[None].expand(K, H, H, 3).contiguous()
    masks = torch.cat([ds.batch(fids[i:i + 8])['mask'] > 0.5 for i in range(0, K, 8)])
    cameras, _, _ = net._cameras(1, dev)
    adj = vertex_adjacency(faces, V)
    # the per-view terms of all K views, resident (what bake_texture computes batch by batch)
    with torch.no_grad():
        defV = []
        for i in range(0, K, args.batch):
            f = fids[i:i + args.batch]
            poses, trans, d_cond, _ = [t.detach() for t in ds.get_grad_parameters(f, dev)]
            defV.append(net.deformer(verts[None].expand(f.numel(), -1, 3), [d_cond, [poses, trans]], ratio=FULL_RATIO))
        defV = torch.cat(defV).contiguous()
        xy_pix = cameras.project(defV)[0].contiguous()
        p2f = torch.cat([rasterize_meshes(*cameras.project_ndc(defV[i:i + args.batch]), faces, H, H).pix_to_face[..., 0] for i in range(0, K, args.batch)])
        p2f = torch.where(p2f >= 0, p2f % F + torch.arange(K, device=dev).view(K, 1, 1) * F, p2f)      # packed over all K views
        normals = vertex_normals(defV, faces, adj)
    tmap = uv_texel_map(vt, ft, R)
    T = int(tmap.tface.shape[0])
    state = {}

    def k_uv():
        uv_texel_map(vt, ft, R)

    def k_vis():
        state["vis"] = face_visibility(p2f, faces, xy_pix, masks)

    def k_alpha():
        state["alpha"] = view_alpha(defV, normals, cameras.cam_pos())

    def k_acc():
        acc = state["acc"]
        acc.slot_cos.fill_(acc.cosv0); acc.slot_view.fill_(-1); acc.count.zero_(); acc.min_cos.fill_(acc.cosv0); acc.min_idx.zero_()
        state["t0"].record()
        acc.accumulate(fids, state["vis"], state["alpha"], xy_pix, images)
        state["t1"].record()

    def k_res():
        state["res"] = state["acc"].resolve(5)

    def k_fill():
        state["tex"] = fill(state["res"].tex_median, state["res"].mask_final, tmap.face >= 0)
    state["acc"] = TextureAccumulator(tmap, faces, 50, 68.)
    state["t0"], state["t1"] = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_end = time.time() + args.warmup_seconds                           # warm-up: the whole chain, until the clock has settled
    n_warm = 0
    while time.time() < t_end or n_warm < 2:
        k_vis(); k_alpha(); k_acc(); k_res(); k_fill()
        torch.cuda.synchronize()
        n_warm += 1
    acc_ms = []
    for _ in range(args.reps):                                          # (the slot reset of k_acc stays outside the event pair)
        k_acc()
        state["t1"].synchronize()
        acc_ms.append(state["t0"].elapsed_time(state["t1"]))
    times = {"sr_uv_rasterize (+ compaction)": _timed(k_uv, args.reps), "sr_face_visibility": _timed(k_vis, args.reps),
             "sr_view_alpha": _timed(k_alpha, args.reps), "sr_texture_accumulate": float(np.median(acc_ms)),
             "sr_texture_resolve": _timed(k_res, args.reps), "sr_texture_fill": _timed(k_fill, args.reps)}
    acc, res = state["acc"], state["res"]
    accepted = int(acc.count.sum())
    nfin = int(res.mask_final.sum())
    filled_final = int(res.count[res.mask_final].sum())
    A, HW, R2 = 50, H * H, R * R
    bytes_ = {
        # vt, ft once; face claimed + written, bary written; the compaction reads face and bary again and writes the lists
        "sr_uv_rasterize (+ compaction)": 8 * 3 * F + 24 * F + R2 * (4 + 4 + 12) + R2 * 16 + T * 20,
        # pix_to_face read, flags written and rewritten, faces + the vertices' pixel positions per view
        "sr_face_visibility": K * (8 * HW + 2 * F + 24 * F + 8 * V),
        "sr_view_alpha": K * V * (12 + 12 + 4),
        # texel list + state, faces once; per view the flags, alpha, pixel positions and the image; 20 bytes per accepted candidate
        "sr_texture_accumulate": T * (16 + 24) + 24 * F + K * (F + 12 * V + 12 * HW) + 20 * accepted,
        # every slot's cosine, the filled slots' colours of mask_final texels, the best slot's view; four outputs
        "sr_texture_resolve": T * (4 * A + 4 + 4 + 21) + 12 * filled_final,
        # tex_median, the two masks, the texture; the dilation's two byte planes; a float4 pyramid of 1/3 of the texels, written and read twice
        "sr_texture_fill": R2 * (12 + 1 + 1 + 12 + 4) + (R2 // 3) * 16 * 4,
    }
    rows = []
    for name, ms in times.items():
        cp = _copy_ms(bytes_[name], args.reps)
        rows.append((name, ms, bytes_[name], bytes_[name] / ms / 1e6, cp, ms / cp))
    # the whole bake through the public interface (includes the deformer, the rasteriser and the host loop)
    views = [(int(f), images[i], masks[i]) for i, f in enumerate(fids.tolist())]
    t0 = time.time()
    bake_texture(net, verts, faces, vt, ft, views, resolution=R)
    torch.cuda.synchronize()
    whole = time.time() - t0
    lines = [f"Texture bake, {torch.cuda.get_device_name(0)}: template {V} vertices / {F} faces, per_face_atlas, {H} x {H} views, R = {R}, K = {K}, "
             f"agg_num 50, normal_ang 68, check_num 5.", "",
             f"Covered texels T = {T} of {R2}; accepted candidates {accepted} ({accepted / max(T, 1):.1f} per texel); mask_final {nfin} texels.",
             f"Median of {args.reps} HIP-event timings after {n_warm} warm-up passes (>= {args.warmup_seconds:.0f} s).  'copy' is a device-to-device "
             "copy that moves the same number of bytes, timed in the same process.", "",
             "| kernel | ms | MB it must move | GB/s | copy ms | kernel / copy |", "|---|---|---|---|---|---|"]
    lines += [f"| {n} | {ms:.3f} | {b / 1e6:.1f} | {gbs:.0f} | {cp:.3f} | {r:.2f} |" for n, ms, b, gbs, cp, r in rows]
    lines += ["", f"bake_texture end to end (deformer, rasteriser, host loop, {K} views in batches of 8, results copied to the host): {whole:.2f} s.",
              "No reference or parent-commit time exists for this stage (texture_mesh_extract.py needs opendr / VideoAvatar / cv2)."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    print(json.dumps({"texture_bench": {n: {"ms": ms, "bytes": b, "gbps": gbs, "copy_ms": cp} for n, ms, b, gbs, cp, _ in rows}, "T": T, "V": V, "F": F,
                      "K": K, "R": R, "accepted": accepted, "mask_final": nfin, "bake_seconds": whole}))


if __name__ == "__main__":
    main()
