"""The host side of the animate stage (selfreconcode_amd/animate.py): resample_motion, read_motion and the parser's refusals; and the
float64 restatement of the pose feature (tests/_posecond_ref.py) against closed forms, so that what the GPU tests compare with is
itself checked."""
import math

import numpy as np
import pytest

import _posecond_ref as ref


def _motion(T, seed=0):
    rng = np.random.default_rng(seed)
    return (0.5 * rng.standard_normal((T, 24, 3))).astype(np.float32), rng.standard_normal((T, 3)).astype(np.float32)


def _about(axis, angles):
    """[T,24,3]: every joint turned about `axis` by angles [T]."""
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.broadcast_to((np.asarray(angles, np.float64)[:, None] * axis)[:, None, :], (len(angles), 24, 3)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ resample_motion
def test_resample_equal_rates_returns_the_input_bits():
    from selfreconcode_amd.animate import resample_motion
    poses, trans = _motion(7)
    poses[2, 3] = [0., 0., 4.]                       # an angle above pi: a copied row is not renormalised
    for fps in (30., 29.97, 12.5):
        got_p, got_t = resample_motion(poses, trans, fps, fps)
        assert got_p.dtype == np.float32 and got_p.tobytes() == poses.tobytes() and got_t.tobytes() == trans.tobytes()
    got_p, got_t = resample_motion(poses.reshape(7, 72), None, 30., 30.)
    assert got_t is None and got_p.tobytes() == poses.tobytes()


def test_resample_midpoint_is_the_half_angle():
    from selfreconcode_amd.animate import resample_motion
    axis = [1., 2., -2.]
    poses = _about(axis, [0.2, 0.6])
    trans = np.asarray([[0., 1., 2.], [1., 3., 2.]], np.float32)
    got_p, got_t = resample_motion(poses, trans, 30., 60.)
    assert got_p.shape == (3, 24, 3) and got_t.shape == (3, 3)
    assert got_p[0].tobytes() == poses[0].tobytes() and got_p[2].tobytes() == poses[1].tobytes()
    assert np.abs(got_p[1].astype(np.float64) - 0.4 * np.asarray(axis) / 3.).max() < 1e-7
    assert np.abs(got_t[1] - [0.5, 2., 2.]).max() < 1e-7


def test_resample_takes_the_short_arc():
    from selfreconcode_amd.animate import resample_motion
    # 0.1 and 2 pi - 0.1 about z are 0.2 apart the short way, and their quaternions have a negative dot product
    poses = _about([0., 0., 1.], [0.1, 2. * math.pi - 0.1])
    got = resample_motion(poses, None, 30., 60.)[0]
    assert np.abs(got[1]).max() < 1e-6                                      # the short arc's midpoint is the identity, the long one's is pi
    # and a quarter of the way: 0.05 about z
    got = resample_motion(poses, None, 30., 120.)[0]
    assert np.abs(got[1].astype(np.float64) - [0., 0., 0.05]).max() < 1e-6


def test_resample_constant_velocity_round_trip():
    from selfreconcode_amd.animate import resample_motion
    angles = 0.07 * np.arange(9)
    poses = _about([0.3, -1., 0.5], angles)
    trans = (np.arange(9)[:, None] * np.asarray([[0.01, 0., -0.02]])).astype(np.float32)
    up_p, up_t = resample_motion(poses, trans, 30., 60.)
    assert up_p.shape[0] == 17
    axis = np.asarray([0.3, -1., 0.5]) / np.linalg.norm([0.3, -1., 0.5])
    assert np.abs(up_p[:, 0].astype(np.float64) - (0.035 * np.arange(17))[:, None] * axis).max() < 2e-7        # (float32 rows)
    back_p, back_t = resample_motion(up_p, up_t, 60., 30.)
    assert back_p.shape == poses.shape
    assert np.abs(back_p.astype(np.float64) - poses).max() <= 1e-12 and np.abs(back_t.astype(np.float64) - trans).max() <= 1e-12
    # a rate that is no multiple: the last frame clamps, nothing past it
    down = resample_motion(poses, trans, 30., 20.)[0]
    assert down.shape[0] == 6 and np.abs(down[1, 0].astype(np.float64) - 0.105 * axis).max() < 2e-7
    with pytest.raises(ValueError, match="positive frame rates"):
        resample_motion(poses, trans, 30., 0.)
    with pytest.raises(ValueError, match="trans"):
        resample_motion(poses, trans[:3], 30., 60.)


# ------------------------------------------------------------------------------------------------ read_motion and the parser
def test_read_motion(tmp_path):
    from selfreconcode_amd.animate import read_motion
    poses, trans = _motion(4)
    path = str(tmp_path / "m.npz")
    np.savez(path, poses=poses.reshape(4, 72).astype(np.float64), trans=trans, fps=25, shape=np.zeros(10))     # smpl_rec.npz's layout and more
    m = read_motion(path)
    assert m['poses'].dtype == np.float32 and m['poses'].shape == (4, 24, 3) and np.array_equal(m['poses'], poses)
    assert np.array_equal(m['trans'], trans) and m['fps'] == 25.
    np.savez(path, poses=poses)
    m = read_motion(path)
    assert m['trans'] is None and m['fps'] is None
    bad = poses.copy()
    bad[1, 2, 0] = np.nan
    for kwargs, message in (({'trans': trans}, "no `poses`"), ({'poses': poses[:, :23]}, r"poses \[T,24,3\] or \[T,72\]"),
                            ({'poses': poses.astype(np.int32)}, r"poses \[T,24,3\]"), ({'poses': poses[:0]}, "T > 0"),
                            ({'poses': poses, 'trans': trans[:3]}, r"trans \[4,3\]"), ({'poses': bad}, "non-finite"),
                            ({'poses': poses, 'trans': trans * np.inf}, "non-finite"), ({'poses': poses, 'fps': 0.}, "fps")):
        np.savez(path, **kwargs)
        with pytest.raises(ValueError, match=message) as e:
            read_motion(path)
        assert path in str(e.value)


def test_parser_refusals(tmp_path, capsys):
    from selfreconcode_amd.animate import build_parser, parse_args
    poses, trans = _motion(6)
    good, bad = str(tmp_path / "good.npz"), str(tmp_path / "bad.npz")
    np.savez(good, poses=poses, trans=trans, fps=60.)
    np.savez(bad, poses=poses[:, :5])
    base = ['--rec-root', 'x', '--motion', good]
    for argv, message in ((['--rec-root', 'x'], "--rec-root and --motion are required"), (['--motion', good], "required"),
                          (base + ['--nI'], "--nI"), (base + ['--cond', 'pose'], "invalid choice"), (base + ['--cond-k', '9'], "--cond-k"),
                          (base + ['--cond-sigma', '0'], "--cond-sigma"), (base + ['--fps-out', '-1'], "--fps-out"),
                          (base + ['--trans', 'mean'], "invalid choice"), (base + ['--video', '--video-quality', '0'], "--video-quality"),
                          (['--rec-root', 'x', '--motion', bad], "poses"), (['--rec-root', 'x', '--motion', str(tmp_path / "none.npz")], "none.npz")):
        with pytest.raises(SystemExit) as e:
            parse_args(build_parser(), argv)
        assert e.value.code == 2 and message in capsys.readouterr().err, argv
    args, motion = parse_args(build_parser(), base + ['--fps-out', '30', '--frames', '2', '--self-check'])
    assert motion['poses'].shape == (2, 24, 3) and motion['fps'] == 30. and args.fps == 30. and args.self_check == 0
    assert motion['poses'].tobytes() == poses[[0, 2]].tobytes() and motion['trans'].tobytes() == trans[[0, 2]].tobytes()
    args, motion = parse_args(build_parser(), base + ['--self-check', '3', '--video', '--fps', '12'])
    assert motion['poses'].shape[0] == 6 and args.fps == 12. and args.self_check == 3 and args.cond == 'blend' and args.cond_exclude == -1


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_closed_forms():
    assert not ref.features(np.zeros((2, 24, 3))).any()                     # zero pose -> zero feature
    rng = np.random.default_rng(3)
    base = 0.4 * rng.standard_normal((1, 24, 3))
    base[0, 7] = 0.
    for a in (1e-3, 0.5, 2., math.pi):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        other = base.copy()
        other[0, 7] = a * axis                                               # one joint, from rest, by the angle a: |R - I|_F^2 = 4 (1 - cos a)
        d2 = ref.distances(ref.features(base), ref.features(other))[0, 0]
        assert abs(d2 - 4. * (1. - math.cos(a))) <= 1e-6 * max(d2, 1e-6)     # (the +1e-8 inside the norm moves the angle by <= 2e-8 relative to a >= 1e-3)
        turned = base.copy()
        turned[0, 0] = [0.3, -2., 1.]                                        # the root joint is not part of the feature
        assert ref.distances(ref.features(base), ref.features(turned))[0, 0] == 0.
    w = np.zeros(23)
    w[6] = 4.                                                                # joint 7 is entry 6 of the weights
    assert abs(ref.distances(ref.features(base, w), ref.features(other, w))[0, 0] - 4. * 4. * (1. - math.cos(math.pi))) < 1e-5
    # neighbours, blend and calibration on numbers small enough to do by hand
    D = np.asarray([[3., 1., np.nan, 1., 0.5]])
    idx, d2 = ref.neighbors(D, 3)
    assert idx.tolist() == [[4, 1, 3]] and d2.tolist() == [[0.5, 1., 1.]]
    idx, d2 = ref.neighbors(D, 8, [4], 1)
    assert idx.tolist() == [[1, 0, -1, -1, -1, -1, -1, -1]] and d2[0, :2].tolist() == [1., 3.] and np.isposinf(d2[0, 2:]).all()
    out, wts = ref.blend(np.asarray([[1, 0, -1], [-1, -1, -1]]), np.asarray([[1., 3., np.inf], [np.inf] * 3]), np.asarray([[2.], [4.]]), 1.)
    e = math.exp(-1.)
    assert np.allclose(wts, [[1. / (1. + e), e / (1. + e), 0.], [0., 0., 0.]]) and np.allclose(out, [[(4. + 2. * e) / (1. + e)], [0.]])
    assert ref.calibrate(np.asarray([4., np.inf, 1., 3., 2.])) == 2. and ref.calibrate(np.asarray([np.inf])) is None
