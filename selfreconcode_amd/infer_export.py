"""The files the reference's infer.py writes (infer.py:102-183), from `OptimNetwork.infer` with the shaded previews on:

    out_root/tmp.ply               the template (ASCII PLY)
    out_root/meshs/<fid>.npy       the posed template vertices [V,3] float32
    out_root/meshs/<fid>.png       the posed, Phong-shaded mesh (imgs)
    out_root/def1meshs/<fid>.png   the template plus the non-rigid offset, seen from the front (def1imgs)
    out_root/colors/<fid>.png      the rendering network's image (with `color`)
    out_root/errors.txt            the per-frame mask error 1 - IoU, in the reference's layout

PNG pixels are the ones cv2.imwrite writes for the reference's arrays (it takes BGR): file RGB = img[..., :3] for the previews
(written as img[:, :, [2, 1, 0]]) and color[..., ::-1] for the colour image (written as is).

With `video=True` each of the three folders also receives `video.avi`, a Motion-JPEG AVI (video.py) of exactly the
pixels its PNGs hold, one frame per visited frame in the order visited: what stands in for the reference's `video.mp4`.
`images=False` leaves the PNGs out (the reference's --nI); meshs/<fid>.npy is written either way, as in the reference.
"""
import os
import struct
import zlib

import numpy as np
import torch

from .mesh_io import write_ply
from .video import FrameVideo


def write_png(path, img):
    """8-bit PNG of a uint8 array [H,W] (grey), [H,W,3] (RGB) or [H,W,4] (RGBA), filter 0 on every row; standard library only."""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, c = a.shape
    ctype = {1: 0, 3: 2, 4: 6}[c]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * c)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0))
                 + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_errors(path, maskE):
    """errors.txt of infer.py:172-181: one line per frame with an error (>= 0), then mean / max / min and the ten largest --
    whose `maxinds` index the array FILTERED to e >= 0 (not frame ids), in numpy's default argsort order, as the reference writes them."""
    maskE = np.asarray(maskE, dtype=np.float64)
    with open(path, "w") as ff:
        ff.write("      mask\n")
        for ind, e in enumerate(maskE.tolist()):
            if e >= 0.:
                ff.write("%4d: %.4f\n" % (ind, e))
        maskE = maskE[maskE >= 0.]
        ff.write("mask mean: %.4f, max: %.4f, min: %.4f, maxinds:" % (maskE.mean(), maskE.max(), maskE.min()))
        for ind in (-maskE).argsort()[:10]:
            ff.write("%d " % ind)


def _frame_count(dataset):
    return len(dataset) if hasattr(dataset, "__len__") else int(dataset.frame_num)


def export_frames(net, TmpVs, Tmpfs, batches, out_root, ratio, color=True, overlay=False, video=False, images=True, fps=30., quality=90):
    """infer.py's loop over `batches` -- (frame_ids, outs) as the reference's dataloader yields them, outs['mask'] [B,H,W] and
    outs['img'] [B,H,W,3] in [-1, 1] (BGR) -- writing the files listed in the module docstring under `out_root`.  color=False is
    --nColor (no colour pass, no colors/*.png), overlay=True is --C (backgrounds from the input images); video / images / fps / quality: the module docstring's
    video.avi files and --nI.  Returns the per-frame mask errors written to errors.txt (-1: frame not visited)."""
    device = TmpVs.device
    ds = net.dataset
    os.makedirs(out_root, exist_ok=True)
    write_ply(os.path.join(out_root, "tmp.ply"), TmpVs.detach().cpu().numpy(), Tmpfs.cpu().numpy())
    for sub in ("colors", "meshs", "def1meshs"):
        os.makedirs(os.path.join(out_root, sub), exist_ok=True)
    maskE = -1. * np.ones((_frame_count(ds),))
    previous = net.shaded_previews
    net.shaded_previews = True
    videos = {sub: FrameVideo(os.path.join(out_root, sub, "video.avi"), device, fps, quality)
              for sub in (("meshs", "def1meshs", "colors") if color else ("meshs", "def1meshs"))} if video else {}
    try:
        for frame_ids, outs in batches:
            frame_ids = torch.as_tensor(frame_ids).long().to(device)
            gts = {'mask': outs['mask'].to(device)}
            if overlay:
                gts['image'] = (outs['img'].to(device) + 1.) / 2.
            colors, imgs, def1imgs, defVs = net.infer(TmpVs, Tmpfs, ds.H, ds.W, ratio, frame_ids, not color, gts)
            fids = frame_ids.cpu().numpy().reshape(-1)
            for fid, img, def1img, defV in zip(fids, imgs, def1imgs, defVs):
                np.save(os.path.join(out_root, "meshs", "%d.npy" % fid), defV.reshape(-1, 3))
                if images:
                    write_png(os.path.join(out_root, "meshs", "%d.png" % fid), img[:, :, :3])
                    write_png(os.path.join(out_root, "def1meshs", "%d.png" % fid), def1img[:, :, :3])
            if colors is not None and images:
                for fid, c in zip(fids, colors):
                    write_png(os.path.join(out_root, "colors", "%d.png" % fid), c[:, :, ::-1])
            if video:
                videos["meshs"].add(np.stack([img[:, :, :3] for img in imgs]))
                videos["def1meshs"].add(np.stack([img[:, :, :3] for img in def1imgs]))
                if colors is not None:
                    videos["colors"].add(np.stack([c[:, :, ::-1] for c in colors]))
            maskE[fids] = gts['maskE']
    finally:
        net.shaded_previews = previous
        for v in videos.values():
            v.close()
    write_errors(os.path.join(out_root, "errors.txt"), maskE)
    return maskE
