#!/usr/bin/env python
"""Times the textured renderer's three kernels at full size: an ellipsoid of ~20 000 faces with a latitude / longitude UV map, a random
R = 1680 texture that is valid on 70 % of a 16-texel checker of blocks, 8 turntable views of 540 x 540.  Per entry: HIP-event time of a
window of --inner launches, median of --reps windows, after a warm-up of at least --warmup-seconds of the same launches (a ten-launch
window measures the clock ramp, not the kernel), the bytes the model below says it moves, and the achieved GB/s.  sr_shade_phong is
timed on the same fragments in the same process as the yardstick: it is the other per-pixel shader of the package, bound by the same
fragment stream.  Prints a markdown table (profiles/textured_render.md holds one run of it) and one JSON line.

Modelled bytes of sr_shade_textured: every pixel streams pix_to_face 8 + bary 12 in and rgba 16 + coverage 4 out = 40 bytes; a covered
pixel also gathers ft 24 + vt 24 + lod 4 + eight 16-byte taps = 180 bytes, most of them from cache (neighbouring pixels share taps).

There is no earlier time to compare with -- the parent commit cannot draw a textured mesh -- and no pass / fail on time.

    python tools/texrender_bench.py [--resolution 1680] [--image 540] [--views 8] [--grid 100] [--out profiles/textured_render_table.md]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ellipsoid(n):
    """A latitude / longitude grid of (n + 1)^2 vertices and 2 n^2 triangles on an ellipsoid, with uv = (longitude, latitude)."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    lat, lon = (i / n - 0.5) * math.pi * 0.98, j / n * 2. * math.pi
    verts = np.stack([0.35 * np.cos(lat) * np.cos(lon), 0.8 * np.sin(lat), 0.25 * np.cos(lat) * np.sin(lon)], -1).reshape(-1, 3)
    vt = np.stack([0.01 + 0.98 * j / n, 0.01 + 0.98 * i / n], -1).reshape(-1, 2)
    a = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)])
    return verts.astype(np.float32), faces.astype(np.int64), vt.astype(np.float32)


def timed(fn, inner, reps, warmup_seconds):
    """(median, min, max) ms per call over `reps` event-timed windows of `inner` calls, after at least `warmup_seconds` of calls, and
    the median host time per call of enqueueing them.  Where the two agree the window measured the host's enqueue rate, not the kernel."""
    t_end = time.time() + warmup_seconds
    while time.time() < t_end:
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
    ms, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        host.append((time.perf_counter() - t0) * 1e3 / inner)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms)), float(np.median(host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=1680)
    ap.add_argument("--image", type=int, default=540)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--grid", type=int, default=100, help="the mesh has 2 grid^2 faces")
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup-seconds", type=float, default=3.0)
    ap.add_argument("--out", default=None, help="also write the markdown table here")
    args = ap.parse_args()
    from selfreconcode_amd.model.CameraMine import RectifiedPerspectiveCameras
    from selfreconcode_amd.ops import rasterize_meshes, shade_phong, vertex_adjacency, vertex_normals
    from selfreconcode_amd.render import turntable_vertices
    from selfreconcode_amd.render_ops import mip_layout, shade_textured, texture_face_lod, texture_mips
    if not torch.cuda.is_available():
        raise SystemExit("texrender_bench: no GPU (there is nothing to time on a CPU)")
    dev = "cuda:0"
    R, S, N = args.resolution, args.image, args.views
    verts, faces, vt = [torch.from_numpy(a).to(dev) for a in ellipsoid(args.grid)]
    ft = faces.clone()
    V, F = verts.shape[0], faces.shape[0]
    gen = torch.Generator(device=dev).manual_seed(0)
    texture = torch.rand((R, R, 3), device=dev, generator=gen)
    blocks = torch.rand(((R + 15) // 16, (R + 15) // 16), device=dev, generator=gen) < 0.7
    valid = blocks.repeat_interleave(16, 0).repeat_interleave(16, 1)[:R, :R].contiguous()
    Rm = torch.tensor([[-1., 0., 0.], [0., 1., 0.], [0., 0., -1.]], device=dev)
    f = 1.25 * S
    cam = RectifiedPerspectiveCameras(torch.tensor([[f, f]], device=dev), torch.tensor([[S / 2., S / 2.]], device=dev), Rm.view(1, 3, 3),
                                      torch.tensor([[0., 0., 2.4]], device=dev), image_size=[(S, S)])
    defV = turntable_vertices(verts, N).contiguous()
    with torch.no_grad():
        frags = rasterize_meshes(*cam.project_ndc(defV), faces, S, S)
        xy_pix = cam.project(defV)[0].contiguous()
        normals = vertex_normals(defV, faces, vertex_adjacency(faces, V))
    campos = cam.cam_pos().view(1, 3).expand(N, 3).contiguous()
    state = {"mips": texture_mips(texture, valid)}
    state["lod"] = texture_face_lod(xy_pix, faces, vt, ft, state["mips"])

    def k_mips():
        state["mips"] = texture_mips(texture, valid)

    def k_lod():
        state["lod"] = texture_face_lod(xy_pix, faces, vt, ft, state["mips"])

    def k_shade():
        state["out"] = shade_textured(frags, ft, vt, state["mips"], state["lod"], return_coverage=True)

    def k_phong():
        state["phong"] = shade_phong(defV, normals, faces, frags, campos)
    pixels = N * S * S
    covered = int((frags.pix_to_face >= 0).sum())
    texels = mip_layout(R)[1][-1] + 1
    lod = state["lod"]
    bytes_ = {
        # texture + valid read, level 0 written; every further level read once and written once
        "sr_texture_mips": R * R * (12 + 1 + 16) + (texels - R * R) * 16 + (texels - 1) * 16,
        # faces, ft once per image (cached after the first), three pixel positions and three uvs per face, one float out
        "sr_texture_face_lod": N * F * (24 + 24 + 24 + 24 + 4),
        "sr_shade_textured": pixels * 40 + covered * 180,
        # pix_to_face, bary, rgba streamed; faces and three positions and normals per covered pixel, camera and light
        "sr_shade_phong": pixels * (8 + 12 + 16) + covered * (24 + 36 + 36 + 24),
    }
    inner = {"sr_texture_mips": max(args.inner // 10, 1), "sr_texture_face_lod": args.inner, "sr_shade_textured": args.inner, "sr_shade_phong": args.inner}
    rows = []
    for name, fn in (("sr_texture_mips", k_mips), ("sr_texture_face_lod", k_lod), ("sr_shade_textured", k_shade), ("sr_shade_phong", k_phong)):
        med, lo, hi, host = timed(fn, inner[name], args.reps, args.warmup_seconds)
        rows.append((name, med, lo, hi, bytes_[name], bytes_[name] / med / 1e6, host))
    rgba, cov = state["out"]
    on = frags.pix_to_face[..., 0] >= 0
    lines = [f"Textured render, {torch.cuda.get_device_name(0)}: ellipsoid of {V} vertices / {F} faces (latitude / longitude UVs), R = {R} "
             f"({len(mip_layout(R)[0])} levels, {texels * 16 / 1e6:.1f} MB of float4 texels), {N} views of {S} x {S}.", "",
             f"Covered pixels {covered} of {pixels} ({covered / pixels:.1%}); face lod mean {float(lod.mean()):.2f}, min {float(lod.min()):.2f}, max "
             f"{float(lod.max()):.2f}; sampled coverage mean {float(cov[on].mean()):.3f}, {float((cov[on] < 0.25).float().mean()):.2%} of the covered pixels below 0.25.",
             f"Median (min .. max) of {args.reps} HIP-event windows of `inner` launches each, after >= {args.warmup_seconds:.0f} s of the same launches.",
             "`host ms` is what the operator takes to enqueue one call (output allocation, argument checks, the launch); where it equals `ms per "
             "call` the queue ran dry, the window measured the host, and the GB/s column is a lower bound on the kernel's rate.", "",
             "| entry | launches per window | ms per call | min .. max | host ms | modelled MB | GB/s |", "|---|---|---|---|---|---|---|"]
    lines += [f"| {n} | {inner[n]} | {ms:.4f} | {lo:.4f} .. {hi:.4f} | {h:.4f} | {b / 1e6:.1f} | {gbs:.0f} |" for n, ms, lo, hi, b, gbs, h in rows]
    t = {r[0]: r[1] for r in rows}
    lines += ["", f"sr_shade_textured / sr_shade_phong on the same fragments, per call as timed above: {t['sr_shade_textured'] / t['sr_shade_phong']:.2f} "
              "(a row whose host ms equals its ms per call is the host's time; kernel against kernel needs a kernel trace of this script: "
              "rocprofv3 --kernel-trace --stats -- python tools/texrender_bench.py --reps 4 --warmup-seconds 1).",
              f"Modelled bytes per pixel of sr_shade_textured: 40 streamed per pixel + 180 gathered per covered pixel = "
              f"{bytes_['sr_shade_textured'] / pixels:.0f} on average here.",
              "No earlier time exists for this stage (the parent commit cannot draw a textured mesh); nothing here is a pass / fail."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    print(json.dumps({"texrender_bench": {n: {"ms": ms, "min_ms": lo, "max_ms": hi, "bytes": b, "gbps": gbs, "host_ms": h} for n, ms, lo, hi, b, gbs, h in rows},
                      "V": V, "F": F, "R": R, "views": N, "image": S, "covered": covered, "pixels": pixels}))


if __name__ == "__main__":
    main()
