"""Times the Motion-JPEG encoder (selfreconcode_amd/video.py, csrc/mjpeg.hip) on the GPU next to what it replaces or competes with on
the host -- infer_export.write_png and PIL's JPEG encoder -- for 540 x 540 and 1080 x 1080 frames of a shaded body on white (the
workload's kind of picture) and of noise (the worst case), and the export loop of `infer --nColor` per frame without videos, with
--video and with --video --nI.  Every figure is the mean over windows that alternate between the candidates after seconds of warm-up
(a short window measures the clock ramp, tools/README.md); stage times are HIP events around each stage's launches.

    python tools/mjpeg_bench.py [--out profiles/mjpeg_encode.json] [--seconds 2.0] [--export-size 540] [--export-frames 8]
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from selfreconcode_amd import video_ops  # noqa: E402
from selfreconcode_amd.infer_export import export_frames, write_png  # noqa: E402
from selfreconcode_amd.video import JpegEncoder  # noqa: E402

HBM_GBS = 8000.
QUALITY = 90


def body_on_white(S, device):
    ax = (torch.arange(S, device=device, dtype=torch.float32) + .5) / S * 2 - 1
    v, u = torch.meshgrid(ax, ax, indexing="ij")
    inside = (u / .45) ** 2 + (v / .9) ** 2 < 1.
    shade = (.75 - .4 * u + .2 * v).clamp(0., 1.)
    tex = torch.randint(-6, 7, (S, S), device=device, generator=torch.Generator(device).manual_seed(7)).float()
    base = torch.tensor([205., 160., 140.], device=device)
    img = (base * shade[..., None] + tex[..., None]).clamp(0., 255.)
    return torch.where(inside[..., None], img, torch.full_like(img, 255.)).to(torch.uint8)


def noise(S, device):
    return torch.randint(0, 256, (S, S, 3), device=device, dtype=torch.uint8, generator=torch.Generator(device).manual_seed(S))


def interleaved(candidates, seconds, windows=5):
    """{name: ms per call}: every candidate warmed for `seconds` / len, then `windows` rounds that time each candidate in turn for as
    many calls as its warm-up made (host clock around calls that end in a synchronise)."""
    calls = {}
    for name, fn in candidates.items():
        t0, n = time.time(), 0
        while time.time() - t0 < seconds / len(candidates) or n < 2:
            fn(); torch.cuda.synchronize(); n += 1
        calls[name] = max(2, n // windows)
    total = {name: 0. for name in candidates}
    for _ in range(windows):
        for name, fn in candidates.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls[name]):
                fn()
            torch.cuda.synchronize()
            total[name] += time.perf_counter() - t0
    return {name: 1e3 * total[name] / (windows * calls[name]) for name in candidates}


def stage_times(enc, frames, runs):
    """ms per call of the three stages, HIP events around `runs` back-to-back calls of each (warm)."""
    B, H, W = frames.shape[:3]
    ws = enc._workspace(B)
    coef = video_ops.jpeg_transform(frames, enc.qtab)
    stages = {"transform": lambda: video_ops.jpeg_transform(frames, enc.qtab), "entropy": lambda: video_ops.jpeg_entropy(coef, H, W, enc.huff, ws),
              "gather": lambda: video_ops.jpeg_gather(B, ws)}
    out = {}
    for name, fn in stages.items():
        fn(); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(runs):
            fn()
        b.record(); torch.cuda.synchronize()
        out[name] = a.elapsed_time(b) / runs
    return out


def encoder_rows(seconds, device):
    rows = []
    for S in (540, 1080):
        for kind, make in (("body", body_on_white), ("noise", noise)):
            one = make(S, device)[None].contiguous()
            eight = one.expand(8, -1, -1, -1).contiguous()
            host = one[0].cpu().numpy()
            enc = JpegEncoder(S, S, QUALITY, device, max_batch=8)
            jpeg = enc.encode(one)[0]
            from PIL import Image
            pil_img = Image.fromarray(host)
            png_path = os.path.join(tempfile.gettempdir(), "mjpeg_bench.png")

            def pil_encode():
                buf = io.BytesIO()
                pil_img.save(buf, "JPEG", quality=QUALITY, subsampling=2, optimize=False)
                return buf.getvalue()
            ms = interleaved({"gpu_b1": lambda: enc.encode(one), "gpu_b8": lambda: enc.encode(eight), "write_png": lambda: write_png(png_path, host),
                              "pil_jpeg": pil_encode, "download_then_nothing": lambda: one.cpu()}, seconds)
            st = stage_times(enc, eight, 50)
            R, M = video_ops.geometry(S, S)
            pixels = 8 * S * S
            moved = {"transform": pixels * 3 + 8 * R * M * 768,                                     # RGB in, coefficients out
                     "entropy": 8 * R * M * 768 + 3 * (len(jpeg) - len(enc.header) - 2) * 8,         # coefficients in; bits written, read, stuffed bytes out
                     "gather": 2 * (len(jpeg) - len(enc.header) - 2) * 8}
            rows.append({"size": S, "kind": kind, "bytes_per_frame": len(jpeg), "pil_bytes_per_frame": len(pil_encode()),
                         "png_bytes_per_frame": os.path.getsize(png_path), "gpu_b1_ms_per_frame": ms["gpu_b1"], "gpu_b8_ms_per_frame": ms["gpu_b8"] / 8,
                         "write_png_ms": ms["write_png"], "pil_jpeg_ms": ms["pil_jpeg"], "download_raw_ms": ms["download_then_nothing"],
                         "stage_ms_b8": st, "stage_gbs_b8": {k: moved[k] / (st[k] * 1e-3) / 1e9 for k in st},
                         "stage_share_of_hbm_b8": {k: moved[k] / (st[k] * 1e-3) / 1e9 / HBM_GBS for k in st}})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def export_rows(S, nframes, seconds, device):
    """ms per frame of infer's export loop (export_frames, color=False: `infer --nColor`) on the synthetic scene at S x S."""
    from selfreconcode_amd.synthetic import build_synthetic_scene
    torch.manual_seed(0)
    net, ds, _ = build_synthetic_scene(device=device, frame_num=nframes, H=S, W=S, resolutions=[(15, 21, 9), (29, 41, 17)],
                                       lbs_volume_shape=(17, 57, 33), consistent_masks=False)
    net.point_radius = 0.03
    ratio = {'sdfRatio': 1., 'deformerRatio': 0.62, 'renderRatio': 1.}
    verts, faces = net.discretizeSDF(ratio, None, 0.0)
    batches = [(torch.tensor([i]), {k: v.cpu() for k, v in ds.batch(torch.tensor([i], device=device)).items()}) for i in range(nframes)]
    root = tempfile.mkdtemp(prefix="mjpeg_bench_")
    modes = {"infer --nColor": {}, "infer --nColor --video": {"video": True}, "infer --nColor --video --nI": {"video": True, "images": False}}
    ms = interleaved({name: (lambda kw=kw: export_frames(net, verts, faces, batches, root, ratio, color=False, quality=QUALITY, **kw))
                      for name, kw in modes.items()}, seconds, windows=3)
    return {"size": S, "frames": nframes, "ms_per_frame": {name: v / nframes for name, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--export-size", type=int, default=540); ap.add_argument("--export-frames", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mjpeg_bench: needs the GPU (a CPU run says nothing about it)")
    device = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "quality": QUALITY, "encoder": encoder_rows(args.seconds, device)}
    if args.export_size > 0:
        res["export"] = export_rows(args.export_size, args.export_frames, args.seconds, device)
        print(json.dumps(res["export"]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
