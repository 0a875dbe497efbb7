"""What selfreconcode_amd/posed.py and video.py state once for every stage after training, without a GPU: the float -> uint8
conversion, the silhouette's 1 - IoU, the all-ones ratio and the video arguments of the infer and render commands."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u8_inputs():
    k = np.arange(256, dtype=np.float32) / np.float32(255.)
    return np.concatenate([k, np.nextafter(k, np.float32(-np.inf)), np.nextafter(k, np.float32(np.inf)),
                           np.array([-1., -0., 1., 1. + 2. ** -23, 300.], np.float32)]).astype(np.float32)


def test_to_u8_is_the_clamp_the_stages_wrote():
    from selfreconcode_amd.posed import to_u8
    x = _u8_inputs()
    assert x.dtype == np.float32 and x.shape == (3 * 256 + 5,) and x[-2] > 1.
    t = torch.from_numpy(x)
    got = to_u8(t)
    assert got.dtype == torch.uint8 and got.device == t.device
    want = torch.clamp(t * 255., min=0., max=255.).numpy().astype(np.uint8)
    np.testing.assert_array_equal(got.numpy(), want)
    # the texture command's host form, folded in: clip then scale
    np.testing.assert_array_equal(got.numpy(), np.uint8(np.clip(x, 0., 1.) * 255))
    np.testing.assert_array_equal(to_u8(x).numpy(), want)                                             # a numpy array is taken as it is
    assert want[0] == 0 and want[255] == 255 and (want[-5:] == [0, 0, 255, 255, 255]).all()
    mask = np.array([[True, False], [False, True]])
    np.testing.assert_array_equal(to_u8(mask).numpy(), np.uint8(np.clip(np.asarray(mask, np.float32), 0., 1.) * 255))
    np.testing.assert_array_equal(to_u8(mask).numpy(), [[255, 0], [0, 255]])


def test_mask_iou_error_is_the_expression_of_infer():
    from selfreconcode_amd.posed import mask_iou_error
    m = torch.zeros(2, 4, 4)
    g = torch.zeros(2, 4, 4)
    m[0, :2], g[0, 2:] = 1., 1.                                                                       # disjoint
    m[1, 1:3, :3] = 1.
    g[1] = m[1]                                                                                       # identical
    N = 2
    want = 1. - (m * g).view(N, -1).sum(1) / (m + g - m * g).abs().view(N, -1).sum(1)
    got = mask_iou_error(m, g)
    assert got.dtype == torch.float32 and got.shape == (2,) and torch.equal(got, want)
    assert got.tolist() == [1., 0.]


def test_full_ratio_is_defined_once():
    from selfreconcode_amd import infer, mesh_prep, posed, render, texture  # noqa: F401
    assert posed.FULL_RATIO == {'sdfRatio': 1., 'deformerRatio': 1., 'renderRatio': 1.}
    assert infer.FULL_RATIO is posed.FULL_RATIO
    hits = []
    for folder, _, names in os.walk(os.path.join(ROOT, "selfreconcode_amd")):
        for name in names:
            if name.endswith(".py"):
                with open(os.path.join(folder, name)) as fh:
                    hits += [(name, ln) for ln in fh if re.search(r"'sdfRatio': 1\.", ln)]
    # (synthetic.py masks its scene at 'deformerRatio': 0.5: a line the pattern finds that is another dict, not a second all-ones one)
    ones = [h for h in hits if not re.search(r"'(deformerRatio|renderRatio)': (?!1\.[,}])", h[1])]
    assert len(ones) == 1 and ones[0][0] == "posed.py", hits
    assert sorted(h[0] for h in hits) == ["posed.py", "synthetic.py"], hits


@pytest.mark.parametrize("command", ["infer", "render"])
def test_video_arguments_of_both_commands(command, capsys):
    import importlib
    from selfreconcode_amd.video import check_video_arguments
    parser = importlib.import_module("selfreconcode_amd." + command).build_parser()
    a = parser.parse_args([])
    assert (a.video, a.fps, a.video_quality) == (False, 30., 90) and isinstance(a.fps, float) and isinstance(a.video_quality, int)
    a = parser.parse_args(['--video', '--fps', '12.5', '--video-quality', '75'])
    assert (a.video, a.fps, a.video_quality) == (True, 12.5, 75)
    check_video_arguments(parser, a)
    check_video_arguments(parser, parser.parse_args(['--video-quality', '0']))                        # without --video nothing is checked
    usage = parser.format_help()
    assert '--fps F' in usage and '--video-quality Q' in usage
    for bad in (['--video', '--video-quality', '0'], ['--video', '--video-quality', '101'], ['--video', '--fps', '0']):
        with pytest.raises(SystemExit):
            check_video_arguments(parser, parser.parse_args(bad))
        assert '--video-quality must lie in 1..100 and --fps must be positive' in capsys.readouterr().err


def test_commands_refuse_a_video_quality_of_zero(tmp_path, capsys):
    from selfreconcode_amd import infer, render
    for main in (infer.main, render.main):
        with pytest.raises(SystemExit):
            main(['--rec-root', str(tmp_path), '--video', '--video-quality', '0'])
        assert '--video-quality must lie in 1..100 and --fps must be positive' in capsys.readouterr().err
    assert os.listdir(tmp_path) == []
