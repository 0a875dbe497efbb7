"""Shared by the reference-parity GPU tests: the PRODUCT side of oracle/scene.py -- the product's modules on the scene's inputs, an
`OptimNetwork` wired from them the way oracle/ref_scene.py wires the reference's, and the train.py loop
(`zero_grad; forward; backward; propagateTmpPsGrad; step`).  What a test asserts, prints or perturbs stays in the test."""
import contextlib
import numpy as np
import torch
from oracle import fixtures as fx
from oracle.scene import adam_over  # noqa: F401   (train.py:139, the same on both sides)

_VOLUME = {}


def lbs_volume_cpu(shape):
    shape = tuple(int(s) for s in shape)
    if shape not in _VOLUME:
        _VOLUME[shape] = fx.synthetic_lbs_volume(shape)          # on the CPU: bit-identical to the reference run's volume
    return _VOLUME[shape]


def product_networks(g_or_lbs_shape, device):
    """(sdf, translator, composite deformer, render net) of the product with the scene's parameters; the skinning-weight volume has the
    shape given, or the golden's `lbs_shape`."""
    from selfreconcode_amd.model.network import getTmpSdf
    from selfreconcode_amd.model.Deformer import MLPTranslator, LBSkinner, CompositeDeformer
    from selfreconcode_amd.model.RenderNet import RenderingNetwork_view_norm
    from selfreconcode_amd.utils import smpl_tmp_Apose
    lbs_shape = g_or_lbs_shape["lbs_shape"] if isinstance(g_or_lbs_shape, dict) else g_or_lbs_shape
    sdf = getTmpSdf(device, 6, 0.6, 256)
    sdf.load_state_dict(fx.sphere_sdf_params(7), strict=True)
    tr = MLPTranslator(128, 6).to(device)
    tr.load_state_dict(fx.det_params(fx.DEF_SPEC, 202, last_scale=0.05), strict=True)
    rn = RenderingNetwork_view_norm(256, 'idr', 9, 3, [512, 512, 512, 512], True, multires_n=0, multires_v=4).to(device)
    rn.load_state_dict(fx.det_params(fx.REND_SPEC, 303), strict=True)
    skin = LBSkinner(lbs_volume_cpu(lbs_shape), fx.LBS_BMIN, fx.LBS_BMAX, fx.synthetic_joints(), np.array(fx.SMPL_PARENTS), init_pose=torch.from_numpy(smpl_tmp_Apose(1)),
                     align_corners=False).to(device)
    return sdf, tr, CompositeDeformer([tr, skin]).to(device), rn


def product_engine(resolutions, device):
    from selfreconcode_amd.MCAcc import Seg3dLossless
    return Seg3dLossless(query_func=None, b_min=fx.LBS_BMIN, b_max=fx.LBS_BMAX, resolutions=[tuple(int(x) for x in r) for r in resolutions], align_corners=False,
                         balance_value=0.0, use_cuda_impl=True).to(device)


def product_net(ds, nets, engine, conf, radius, ang_thr, V0, faces, remesh_intersect=None, first_remesh=None):
    """OptimNetwork on `nets` = product_networks(...) with the template (V0, faces) in place.  `first_remesh`: the index of the first
    call at which forward remeshes; None: the template stays (forward_time = 1)."""
    from selfreconcode_amd.model.optim_network import OptimNetwork
    from selfreconcode_amd.utils import DCTNullSpace
    sdf, _, comp, rn = nets
    dev = next(sdf.parameters()).device
    net = OptimNetwork(sdf, comp, engine, None, rn, conf=conf).to(dev)
    net.dataset = ds
    net.dctnull = DCTNullSpace(10, 30).to(dev)
    net.point_radius, net.angThred = float(radius), float(ang_thr)
    net.TmpVs, net.Tmpfs = V0.to(dev).clone().requires_grad_(True), faces.to(dev)
    net.TmpOptimizer = torch.optim.SGD([net.TmpVs], lr=0.05, momentum=0.9)
    if first_remesh is None:
        net.forward_time = 1
    else:
        net.remesh_intersect = int(remesh_intersect)
        net.forward_time = net.remesh_intersect - int(first_remesh)
    return net


@contextlib.contextmanager
def deferred_param_grads():
    """The mode bench.py runs: weight gradients deferred to one flush."""
    from selfreconcode_amd import mlp_engine
    mlp_engine.set_deferred_param_grads(True)
    try:
        yield
    finally:
        mlp_engine.set_deferred_param_grads(False)


def train_iteration(net, opt, obs, SP, ratio, fids, rand, debug=None, before_forward=None):
    """train.py:162-170.  before_forward(): runs between zero_grad and forward (a remesh done by hand, say).  Returns the loss."""
    opt.zero_grad(set_to_none=True)
    if before_forward is not None:
        before_forward()
    loss = net(obs, SP, ratio, fids, rand=rand, debug=debug)
    loss.backward()
    net.propagateTmpPsGrad(fids, ratio)
    opt.step()
    return loss
