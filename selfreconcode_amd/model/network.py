"""SDF network -- drop-in for model/network.py::ImplicitNetwork / getTmpSdf (lines 14-118).

Same constructor, parameter names (`linK.weight_g / weight_v / bias`, so reference checkpoints
load unchanged), call signature `forward(input[P,3], ratio)` -> [P,1] with the 256-d feature left
in `self.rendcond`, and `.gradient()`.  The arithmetic runs on the fp32-MFMA layer kernels:
positional encoding + concat, nine weight-normed linears, Softplus(beta=100) and the skip
`cat([x, PE])/sqrt(2)` are fused into GEMM prologues/epilogues (see mlp_engine.py).
"""
import numpy as np
import torch
import torch.nn as nn

from .Embedder import embed_rows
from ..mlp_engine import MLPSpec, mlp_apply, pad_cols, pad4, pack_linear, input_grads_only
from ..utils.utils import resolve_band_weights


def effective_weight(lin):
    """W = g * v / ||v|| (weight_norm, dim=0) or the plain weight; the reference recomputes this in a
    forward pre-hook at every call (network.py:65-66)."""
    if hasattr(lin, "weight_g"):
        return torch._weight_norm(lin.weight_v, lin.weight_g, 0)
    return lin.weight


class ImplicitNetwork(nn.Module):
    def __init__(self, feature_vector_size, d_in, d_out, dims, geometric_init=True, bias=1.0, skip_in=(), weight_norm=True,
                 multires=0):
        super().__init__()
        assert d_in == 3 and multires > 0, "the HIP path implements the reference's configuration (xyz input with PE)"
        dims = [d_in] + dims + [d_out + feature_vector_size]
        self.d_out = d_out
        self.multires = multires
        dims[0] = 3 + 6 * multires
        self.num_layers = len(dims)
        self.skip_in = tuple(skip_in)
        assert len(set(dims[1:-1])) == 1 and all(0 < s < self.num_layers - 1 for s in self.skip_in) and len(self.skip_in) <= 1
        for l in range(0, self.num_layers - 1):
            out_dim = dims[l + 1] - dims[0] if l + 1 in self.skip_in else dims[l + 1]
            lin = nn.Linear(dims[l], out_dim)
            if geometric_init:                      # network.py:49-63 (sphere of radius `bias`)
                if l == self.num_layers - 2:
                    torch.nn.init.normal_(lin.weight, mean=np.sqrt(np.pi) / np.sqrt(dims[l]), std=0.0001)
                    torch.nn.init.constant_(lin.bias, -bias)
                elif l == 0:
                    torch.nn.init.constant_(lin.bias, 0.0)
                    torch.nn.init.constant_(lin.weight[:, 3:], 0.0)
                    torch.nn.init.normal_(lin.weight[:, :3], 0.0, np.sqrt(2) / np.sqrt(out_dim))
                elif l in self.skip_in:
                    torch.nn.init.constant_(lin.bias, 0.0)
                    torch.nn.init.normal_(lin.weight, 0.0, np.sqrt(2) / np.sqrt(out_dim))
                    torch.nn.init.constant_(lin.weight[:, -(dims[0] - 3):], 0.0)
                else:
                    torch.nn.init.constant_(lin.bias, 0.0)
                    torch.nn.init.normal_(lin.weight, 0.0, np.sqrt(2) / np.sqrt(out_dim))
            if weight_norm:
                lin = nn.utils.weight_norm(lin)
            setattr(self, "lin" + str(l), lin)
        self.spec = MLPSpec.sdf(multires, dims[1], self.num_layers - 1, self.skip_in, dims[-1])
        last = self.spec.layers[-1]
        self.spec_sdf_only = MLPSpec(self.spec.layers[:-1] + [type(last)(last.K, d_out, last.act)], self.spec.K0)
        self.rendcond = None

    def packed_weights(self):
        from ..mlp_engine import packed_weights_of
        return packed_weights_of(self, len(self.spec.layers))

    def forward(self, input, ratio=None, sdf_only=False):
        """`sdf_only=True` (extension): evaluate only the d_out distance rows of the last layer -- for callers that never
        read `rendcond` (mask/eikonal terms, refiner, volume queries): skips 256 of its 257 output rows."""
        ratio = ratio if type(ratio) == float or type(ratio) == int or ratio is None else ratio['sdfRatio']
        A0 = embed_rows(input, self.multires, resolve_band_weights(self.multires, ratio))
        Ws, bs = self.packed_weights()
        if sdf_only:
            self.rendcond = None
            return mlp_apply(self.spec_sdf_only, A0, Ws[:-1] + [Ws[-1][:self.d_out]], bs[:-1] + [bs[-1][:self.d_out]])
        x = mlp_apply(self.spec, A0, Ws, bs)
        if x.shape[-1] > self.d_out:
            self.rendcond = x[:, self.d_out:]
            x = x[:, 0:self.d_out]
        else:
            self.rendcond = None
        return x

    def gradient(self, x, y=None):
        x.requires_grad_(True)
        if y is None:
            y = self.forward(x)
        d_output = torch.ones_like(y, requires_grad=False, device=y.device)
        with input_grads_only():
            gradients = torch.autograd.grad(outputs=y, inputs=x, grad_outputs=d_output, create_graph=True, retain_graph=True,
                                            only_inputs=True)[0]
        return gradients.view(-1, 3)


def getTmpSdf(device, multires, bias=0.6, feature_vector_size=256):
    net = ImplicitNetwork(feature_vector_size=feature_vector_size, d_in=3, d_out=1, dims=[512] * 8, geometric_init=True, bias=bias,
                          skip_in=[4], weight_norm=True, multires=multires)
    return net.to(device)


# ------------------------------------------------------------------------------------------------
# The entry of train.py / infer.py (model/network.py:828-909)
def uniform_vertex_normals(verts, faces):
    """Vertex normals [V,3] as openmesh's update_normals gives them for the reference's tmpBodyNs (network.py:899-903): the UNIT face
    normals summed over a vertex's faces, then normalised -- not the area-weighted normals of the shader (ops.vertex_normals).
    Restated from openmesh's documented default, unpinned.  Once per subject on a body of a few thousand vertices, as in
    the reference: computed on the host in float64 (a sequential index_add: the same bits every time) and returned as float64 on
    the device of `verts`: openmesh hands the reference a float64 array, and the buffer keeps that dtype."""
    v, f = verts.detach().double().cpu(), faces.long().cpu()
    fn = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
    fn = fn / fn.norm(dim=1, keepdim=True).clamp_min(1e-300)
    n = torch.zeros_like(v).index_add_(0, f.reshape(-1), fn.repeat_interleave(3, 0))
    return (n / n.norm(dim=1, keepdim=True).clamp_min(1e-300)).to(verts.device)


SKINNER_RESOLUTION = (128 + 1, 224 + 1, 64 + 1)             # network.py:850


def getOptNet(dataset, N, bmins, bmaxs, resolutions, device, conf, use_initial_sdf=True, use_initial_skinner=True,
              skinner_resolution=SKINNER_RESOLUTION):
    """(optNet, sdf_initialized) as model/network.py:828-909 builds them from a data folder: the SDF (from
    `initial_sdf_idr_<multires>_<pose>.pth` under dataset.root when present: sdf_initialized = -1; else train.initial_iters, or 1200
    when that is not positive), the skinner (from `initial_skinner_<pose>.pth`, else built by initialLBSkinner at `skinner_resolution`
    and written there), translator, render net and Seg3dLossless engine over the skinner's box, with tmpBodyVs / tmpBodyFs / tmpBodyNs
    as buffers.  The body model is dataset.smpl_model (a path, a dict of arrays or an SMPL) when the dataset has one, else
    getSMPL(dataset.gender).  `N` (the batch size the reference builds its cameras for) is unused: cameras are built per call from
    the dataset.  bmins / bmaxs None: the adaptive box."""
    import os.path as osp
    from ..MCAcc import Seg3dLossless
    from ..utils import utils
    from ..utils.checkpoint import load_initial_skinner, save_initial_skinner
    from . import RenderNet
    from .Deformer import CompositeDeformer, getTranslatorNet, initialLBSkinner
    from .optim_network import OptimNetwork
    device = torch.device(device)
    sdf_multires = conf.get_int('sdf_net.multires')
    tmpSdf = getTmpSdf(device, sdf_multires, 0.6, conf.get_int('render_net.condlen'))
    sdf_initialized = conf.get_int('train.initial_iters')
    init_pose_type = conf.get_int('train.skinner_pose_type') if 'train.skinner_pose_type' in conf else 0
    initial_sdf_file = osp.join(dataset.root, 'initial_sdf_idr_%d_%d.pth' % (sdf_multires, init_pose_type))
    if osp.isfile(initial_sdf_file) and use_initial_sdf:
        tmpSdf.load_state_dict(torch.load(initial_sdf_file, map_location='cpu'))
        sdf_initialized = -1
    elif sdf_initialized <= 0:
        sdf_initialized = 1200
    skinner_pth_name = osp.join(dataset.root, 'initial_skinner_%d.pth' % init_pose_type)
    if osp.isfile(skinner_pth_name) and use_initial_skinner:
        skinner, tmpBodyVs, tmpBodyFs = load_initial_skinner(skinner_pth_name)
    else:
        # the rest pose is an A pose, to save volume space
        initPose = torch.from_numpy(utils.smpl_tmp_Apose(init_pose_type)).float().view(1, 24, 3).to(device)
        smpl = getattr(dataset, 'smpl_model', None)
        if smpl is not None and not isinstance(smpl, torch.nn.Module):
            from ..smpl_pytorch import SMPL
            smpl = SMPL(smpl, obj_saveable=True)
        skinner, tmpBodyVs, tmpBodyFs = initialLBSkinner(getattr(dataset, 'gender', None), dataset.shape.detach().to(device), initPose,
                                                         tuple(skinner_resolution), bmins, bmaxs, smpl=smpl)
        save_initial_skinner(skinner_pth_name, skinner, tmpBodyVs, tmpBodyFs)
    deformer = CompositeDeformer([getTranslatorNet(device, conf.get_config('mlp_deformer')), skinner]).to(device)
    engine = Seg3dLossless(query_func=None, b_min=skinner.b_min.view(-1).tolist(), b_max=skinner.b_max.view(-1).tolist(), resolutions=resolutions,
                           align_corners=False, balance_value=0.0, use_cuda_impl=True).to(device)
    rendnet = RenderNet.getRenderNet(device, conf.get_config('render_net'))
    optNet = OptimNetwork(tmpSdf, deformer, engine, None, rendnet, conf=conf.get_config('loss_coarse'))
    optNet.remesh_intersect = conf.get_int('train.coarse.point_render.remesh_intersect')
    optNet.point_radius = conf.get_float('train.coarse.point_render.radius')
    tmpBodyVs, tmpBodyFs = tmpBodyVs.to(device), tmpBodyFs.to(device)
    optNet.register_buffer('tmpBodyVs', tmpBodyVs)
    optNet.register_buffer('tmpBodyFs', tmpBodyFs)
    optNet.register_buffer('tmpBodyNs', uniform_vertex_normals(tmpBodyVs, tmpBodyFs))
    optNet = optNet.to(device)
    optNet.dataset = dataset
    if dataset.poses.requires_grad or dataset.trans.requires_grad:
        optNet.dctnull = utils.DCTNullSpace(10, 30).to(device)
    return optNet, sdf_initialized
