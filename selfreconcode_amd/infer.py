"""The inference driver: the reference's infer.py over infer_export.export_frames.

    python -m selfreconcode_amd.infer --gpu-ids 0 --rec-root <capture folder>/result [--frames N] [--nColor] [--C]
                                      [--video [--fps F] [--video-quality Q] [--nI]]

Reads rec_root/config.conf, opens the capture folder rec_root/.. in order (shuffle off, nothing learnable), loads rec_root/latest.pth,
extracts the template with discretizeSDF(ratio, None, 0.) and writes what infer_export lists under rec_root.

`--video` adds meshs/video.avi, def1meshs/video.avi and (unless --nColor) colors/video.avi: Motion-JPEG encoded on the GPU (video.py,
DESIGN 3.17) at --fps (30) and --video-quality (90), the stand-in for the reference's video.mp4.  Without it no video is
written and the command says so once, with or without `--nV`; `--video --nV` contradict each other and are refused.  `--nI` (no PNGs)
is honoured with --video and refused without it, as the reference refuses --nV --nI: something has to be written.
"""
import argparse
import os.path as osp

import torch

from .config import load_config
from .posed import FULL_RATIO
from .video import add_video_arguments, check_video_arguments

# infer.py:47-53
RESOLUTIONS = [(14 + 1, 20 + 1, 8 + 1), (28 + 1, 40 + 1, 16 + 1), (56 + 1, 80 + 1, 32 + 1), (112 + 1, 160 + 1, 64 + 1), (224 + 1, 320 + 1, 128 + 1)]


def build_parser():
    parser = argparse.ArgumentParser(prog='python -m selfreconcode_amd.infer', description='neu video body infer')
    parser.add_argument('--gpu-ids', nargs='+', type=int, metavar='IDs', default=[0], help='gpu ids')
    parser.add_argument('--batch-size', default=1, type=int, metavar='IDs', help='batch size')
    parser.add_argument('--rec-root', default=None, metavar='M', help='data root')
    parser.add_argument('--frames', default=-1, type=int, metavar='frames', help='render frame nums')
    parser.add_argument('--nV', action='store_true', help='not save video')
    parser.add_argument('--nI', action='store_true', help='not save image')
    parser.add_argument('--C', action='store_true', help='overlay on gtimg')
    parser.add_argument('--nColor', action='store_true', help='not render images')
    add_video_arguments(parser)
    return parser


def parse_args(parser, argv):
    """The arguments, or the parser's error exit for combinations that leave nothing to write or contradict each other."""
    args = parser.parse_args(argv)
    if args.rec_root is None:
        parser.error('--rec-root is required')
    if args.video and args.nV:
        parser.error('--video and --nV contradict each other')
    if args.nI and not args.video:
        parser.error('--nI: the images are all this command writes (videos are not written, see --nV)')
    check_video_arguments(parser, args)
    return args


def limited(dataloader, batch_size, frames, out=None, no_color=False):
    """The loader's batches up to the reference's cut (infer.py:133: stop at the first batch with data_index * batch_size > frames,
    when frames >= 0), announcing each batch's first frame number as the reference prints it."""
    for data_index, batch in enumerate(dataloader):
        if frames >= 0 and data_index * batch_size > frames:
            break
        if out is not None:
            out(data_index * batch_size) if no_color else out(data_index * batch_size, end='\t')
        yield batch


def load_network(rec_root, device="cuda:0", batch_size=1, out=print, resolutions=None):
    """-> (optNet, dataset, dataloader): the capture folder rec_root/.. opened in order (shuffle off, nothing learnable), the network
    of rec_root/config.conf with rec_root/latest.pth loaded, in eval mode.  What `infer` and the texture command start from."""
    from .dataset import getDatasetAndLoader
    from .model import getOptNet
    from .utils.checkpoint import load_model
    device = torch.device(device)
    config = load_config(osp.join(rec_root, 'config.conf'))
    condlen = {'deformer': config.get_int('mlp_deformer.condlen'), 'renderer': config.get_int('render_net.condlen')}
    dataset, dataloader = getDatasetAndLoader(osp.normpath(osp.join(rec_root, osp.pardir)), condlen, batch_size, False,
                                              config.get_int('train.num_workers'), False, False, False, device=device)
    optNet, _ = getOptNet(dataset, batch_size, None, None, resolutions or RESOLUTIONS, device, config)
    out('load model: ' + osp.join(rec_root, 'latest.pth'))
    optNet, dataset = load_model(osp.join(rec_root, 'latest.pth'), optNet, dataset, device)
    optNet.dataset = dataset
    optNet.eval()
    return optNet, dataset, dataloader


def infer(rec_root, device="cuda:0", batch_size=1, frames=-1, color=True, overlay=False, out=print, resolutions=None, video=False, images=True,
          fps=30., quality=90):
    """-> (maskE, TmpVs, Tmpfs, optNet).  `resolutions`: the extraction pyramid instead of infer.py's (small scenes); video, images, fps,
    quality: see infer_export.export_frames."""
    from .infer_export import export_frames
    optNet, dataset, dataloader = load_network(rec_root, device, batch_size, out, resolutions)
    TmpVs, Tmpfs = optNet.discretizeSDF(FULL_RATIO, None, 0.)
    maskE = export_frames(optNet, TmpVs, Tmpfs, limited(dataloader, batch_size, frames, out, not color), rec_root, FULL_RATIO, color=color, overlay=overlay,
                          video=video, images=images, fps=fps, quality=quality)
    out('done')
    return maskE, TmpVs, Tmpfs, optNet


def main(argv=None, out=print, resolutions=None):
    args = parse_args(build_parser(), argv)
    if not args.video:
        out('videos (meshs/video.mp4, def1meshs/video.mp4, colors/video.mp4) are not written' + ('' if args.nV else '; pass --nV to say so'))
    infer(args.rec_root, torch.device('cuda', args.gpu_ids[0]), args.batch_size, args.frames, color=not args.nColor, overlay=args.C, out=out,
          resolutions=resolutions, video=args.video, images=not args.nI, fps=args.fps, quality=args.video_quality)
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
