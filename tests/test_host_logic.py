"""CPU-only tests of the host logic: config parser, Seg3dLossless bookkeeping (pure torch, device agnostic),
synthetic-input determinism, tangent-interleaving helpers."""
import os
import numpy as np
import torch
from oracle import fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_config_matches_the_documented_values():
    from selfreconcode_amd.config import default_config, parse_hocon
    d = default_config()
    assert d.get_int('train.sample_pix_num') == 2048 and d.get_float('loss_coarse.def_regu.c') == 0.5
    assert d.get_int('loss_fine.sample_pix_num') == 6144 and 'pc_weight.mask_weight' not in d.get_config('loss_coarse')
    c = parse_hocon('a { b = 3\n c = "x"\n l = [\n 1\n 2\n ]\n d { e = -0.5 } }\n f = true')
    assert c.get_int('a.b') == 3 and c.get_string('a.c') == 'x' and c.get_list('a.l') == [1, 2] and c.get_float('a.d.e') == -0.5 and c.get_bool('f')


def test_seg3d_bookkeeping_reproduces_the_reference_run(golden):
    from selfreconcode_amd.MCAcc.seg3d_lossless import Seg3dLossless
    g = golden("seg3d")

    def ell(points):
        c = torch.tensor([0.05, -0.1, 0.02]).view(1, 1, 3); a = torch.tensor([0.45, 0.8, 0.25]).view(1, 1, 3)
        return (((points - c) / a).norm(dim=-1) - 1.0).view(1, 1, -1) * 0.25
    eng = Seg3dLossless(ell, [-0.8, -1.25, -0.4], [0.8, 0.95, 0.4], [(5, 7, 3), (9, 13, 5), (17, 25, 9), (33, 49, 17)], balance_value=0.0)
    vol = eng.forward()
    assert eng.stats["queries"] == int(g["nq"]) and torch.equal(vol[0, 0], g["vol"])


def test_synthetic_inputs_are_pure_functions():
    a, b = fx.det_tensor((5, 7), 3, 2.0), fx.det_tensor((5, 7), 3, 2.0)
    assert torch.equal(a, b) and float(a.abs().max()) <= 2.0 and not torch.equal(a, fx.det_tensor((5, 7), 4, 2.0))
    sd = fx.sphere_sdf_params(7)
    assert sd["lin3.weight_v"].shape == (473, 512) and sd["lin8.weight_v"].shape == (257, 512) and abs(float(sd["lin8.bias"][0]) + 0.6) < 1e-6
    vol = fx.synthetic_lbs_volume((5, 6, 7))
    assert vol.shape == (1, 24, 5, 6, 7) and torch.allclose(vol.sum(1), torch.ones(1, 5, 6, 7), atol=1e-5)


def test_mlp_spec_shapes_match_the_reference_layers():
    from selfreconcode_amd.mlp_engine import MLPSpec, pad4
    s = MLPSpec.sdf()
    assert [(l.K, l.N, l.nfill) for l in s.layers] == [(39, 512, 0), (512, 512, 0), (512, 512, 0), (512, 473, 39), (512, 512, 0),
                                                       (512, 512, 0), (512, 512, 0), (512, 512, 0), (512, 257, 0)]
    d = MLPSpec.relu_mlp(167, [512, 512, 512, 512, 3])
    assert [(l.K, l.N) for l in d.layers] == [(167, 512), (512, 512), (512, 512), (512, 512), (512, 3)] and pad4(167) == 168
    flops = sum(2 * l.K * l.N for l in s.layers)
    assert flops == 3933184


def test_state_dict_keys_match_the_reference_modules():
    """checkpoint contract (utils/utils.py:257-289): same parameter/buffer names and shapes as the reference's modules
    (tests/golden/state_keys.json is dumped from the reference's own classes by oracle/gen_golden.py)."""
    import json
    from selfreconcode_amd.model.network import getTmpSdf
    from selfreconcode_amd.model.Deformer import MLPTranslator, LBSkinner
    from selfreconcode_amd.model.RenderNet import RenderingNetwork_view_norm
    from selfreconcode_amd.utils import smpl_tmp_Apose
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "state_keys.json")))
    skin = LBSkinner(fx.synthetic_lbs_volume((7, 11, 9)), fx.LBS_BMIN, fx.LBS_BMAX, fx.synthetic_joints(), np.array(fx.SMPL_PARENTS),
                     init_pose=torch.from_numpy(smpl_tmp_Apose(1)), align_corners=False)
    mods = {"sdf": getTmpSdf("cpu", 6, 0.6, 256), "translator": MLPTranslator(128, 6),
            "render": RenderingNetwork_view_norm(256, 'idr', 9, 3, [512] * 4, True, multires_n=0, multires_v=4), "skinner": skin}
    for name, m in mods.items():
        ours = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert ours == ref[name], (name, set(ours) ^ set(ref[name]))


def test_checkpoint_roundtrip(tmp_path):
    from selfreconcode_amd.utils.checkpoint import save_model, load_model

    class DS:
        frame_num = 4
        poses = torch.zeros(4, 24, 3, requires_grad=True); trans = torch.ones(4, 3, requires_grad=True); shape = torch.zeros(10)
        conds = [torch.randn(4, 128).requires_grad_(), torch.randn(4, 256).requires_grad_()]
        camera_params = {'focal_length': torch.tensor([600., 600.]), 'princeple_points': torch.tensor([270., 270.]),
                         'cam2world_coord_quat': torch.tensor([0., 0., 1., 0.]), 'world2cam_coord_trans': torch.tensor([0., 0., 2.4])}
    from selfreconcode_amd.model.network import getTmpSdf

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.sdf = getTmpSdf("cpu", 6, 0.6, 256)
    a, b = Net(), Net()
    a.sdf.load_state_dict(fx.sphere_sdf_params(3))
    ds = DS()
    path = str(tmp_path / "latest.pth")
    save_model(path, 7, a, ds)
    saved = torch.load(path)
    assert saved["epoch"] == 7 and "sdf.lin3.weight_g" in saved["model_state_dict"] and set(ds.camera_params) <= set(saved)
    ds2 = DS(); ds2.trans = torch.zeros(4, 3, requires_grad=True)
    load_model(path, b, ds2, "cpu")
    assert torch.equal(b.sdf.lin5.weight_v, a.sdf.lin5.weight_v) and torch.equal(ds2.trans, ds.trans) and ds2.trans.requires_grad


def test_pack_cache_follows_parameter_changes():
    """mlp_engine.packed_weights_of hands the previous packs out again only while nothing they were made from has changed: an
    in-place update (optimizer step), a replaced parameter and a replaced layer must each be seen (deferred mode, where the cache is on;
    CPU tensors: the packing itself is plain torch here)."""
    import torch
    import torch.nn as nn
    from selfreconcode_amd import mlp_engine as me

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.lin0 = nn.utils.weight_norm(nn.Linear(7, 12))
            self.lin1 = nn.Linear(12, 3)
    net = Net()
    me.set_deferred_param_grads(True)
    try:
        W0, b0 = me.packed_weights_of(net, 2)            # first call: the autograd packs (not cached)
        W1, b1 = me.packed_weights_of(net, 2)            # entries exist now: plain packs, cached from here on
        W2, b2 = me.packed_weights_of(net, 2)
        assert all(a is b for a, b in zip(W1, W2)) and '_sr_packs' in net.__dict__
        eff = torch._weight_norm(net.lin0.weight_v, net.lin0.weight_g, 0)
        assert torch.allclose(W2[0][:, :7], eff) and torch.allclose(W2[1][:, :12], net.lin1.weight)
        with torch.no_grad():                             # an optimizer step: in place, version bump
            net.lin1.weight.mul_(2.0)
        W3, _ = me.packed_weights_of(net, 2)
        assert torch.allclose(W3[1][:, :12], net.lin1.weight)
        assert W2[1].data_ptr() not in me._ENTRY_BY_PTR and W3[1].data_ptr() in me._ENTRY_BY_PTR      # the replaced entry left the registry
        net.lin1.bias = nn.Parameter(torch.full((3,), 0.25))          # a replaced parameter
        _, b4 = me.packed_weights_of(net, 2)
        assert b4[1] is net.lin1.bias
        net.lin1 = nn.Linear(12, 3)                                    # a replaced layer
        W5, b5 = me.packed_weights_of(net, 2)
        assert torch.allclose(W5[1][:, :12], net.lin1.weight) and b5[1] is net.lin1.bias
    finally:
        me.set_deferred_param_grads(False)


def test_segmented_first_layer_bias_is_validated():
    import pytest
    import torch
    from selfreconcode_amd import mlp_engine as me
    assert me._bias_segments(None, 12, 1) is None and me._bias_segments(torch.zeros(8), 12, 1) is None
    assert me._bias_segments(torch.zeros(3, 8), 12, 1) == (3, 4) and me._bias_segments(torch.zeros(3, 8), 24, 4) == (3, 8)
    with pytest.raises(RuntimeError):
        me._bias_segments(torch.zeros(5, 8), 12, 1)       # rows not divisible by the segments
    with pytest.raises(RuntimeError):
        me._bias_segments(torch.zeros(3, 8), 18, 4)       # a segment that would split a (primal, tangents) group


def test_hoisted_first_layer_wants_one_code_per_frame():
    """The frame-major deformer batch pairs row segment s with bias row s (mlp_engine._bias_segments): a code tensor with another
    number of rows than the batch has frames must not be accepted (the reference's cat of points and expanded codes, Deformer.py:58-61, raises for it)."""
    import pytest
    from selfreconcode_amd.model.Deformer import MLPTranslator
    tr = MLPTranslator(128, 6)
    spec, W0p, Bf = tr.hoisted_first_layer(torch.zeros(3, 128), 3)
    assert W0p.shape == (512, 40) and Bf.shape == (3, 512) and spec.K0 == 39
    with pytest.raises(ValueError):
        tr.hoisted_first_layer(torch.zeros(1, 128), 3)
    with pytest.raises(ValueError):
        tr.hoisted_first_layer(torch.zeros(6, 128), 3)
