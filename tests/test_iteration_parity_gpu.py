"""GPU parity of the mask-loss branch (computeTmpPcLoss, model/network.py:647-697) and of ONE WHOLE training iteration
(forward :451-644 + backward + propagateTmpPsGrad :702-814) against the CPU restatement oracle/iteration_oracle.py, with
every random draw injected on both sides (`rand=`).  ~1.5k template vertices, 2 frames, ~200 rays.

Tolerances: loss terms 1e-4 relative; first-order gradients 1e-3 of the largest entry; gradients that went through
second-order graphs or are sums over all points of a frame 2e-3 of the largest entry (fp32 MFMA / wave-level partial sums
against sequential CPU sums)."""
import numpy as np
import pytest
import torch
from oracle import torch_oracle as orc
from oracle import iteration_oracle as ito
from oracle import fixtures as fx
from oracle import scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIO = {'sdfRatio': 1., 'deformerRatio': 0.62, 'renderRatio': 1.}
H = W = 96


def _scene():
    from selfreconcode_amd.synthetic import build_synthetic_scene
    torch.manual_seed(0)
    net, ds, conf = build_synthetic_scene(device=DEV, frame_num=40, H=H, W=W, resolutions=[(15, 21, 9), (29, 41, 17)],
                                          lbs_volume_shape=(17, 57, 33), consistent_masks=False)
    net.point_radius = 0.03
    with torch.no_grad():                                   # a deformation field that does something (default init: offsets ~1e-3)
        net.deformer.defs[0].lin4.weight.mul_(20.0)
    return net, ds, conf


def _oracle_scene(net, ds):
    cp = lambda sd: {k: v.detach().cpu().clone().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point}
    skin = net.deformer.defs[1]
    sk = dict(ws=skin.ws.detach().cpu().contiguous(), b_min=skin.b_min.cpu().view(3), b_max=skin.b_max.cpu().view(3), Js=skin.Js.cpu(),
              init_pose=skin.init_pose.cpu())
    leaf = lambda t: t.detach().cpu().clone().requires_grad_(True)
    q = ds.camera_params['cam2world_coord_quat'].detach().cpu().view(1, 4)
    camleaf = lambda t: t.detach().cpu().clone().requires_grad_(t.requires_grad)      # the intrinsics / T are optimised (config.conf:10-15)
    cam = dict(focal=camleaf(ds.camera_params['focal_length']), princ=camleaf(ds.camera_params['princeple_points']), R=orc.quat2mat(q)[0],
               T=camleaf(ds.camera_params['world2cam_coord_trans']), H=H, W=W)
    tr_sd = {k: v for k, v in net.deformer.defs[0].state_dict().items()}
    return ito.Scene(cp(net.sdf.state_dict()), cp(tr_sd), cp(net.netRender.state_dict()), sk, leaf(ds.poses), leaf(ds.trans), leaf(ds.conds[0]),
                     leaf(ds.conds[1]), cam, net.conf, net.point_radius, net.angThred)


def close(a, b, rtol=1e-3, frac=1e-3, name=""):
    a = a.detach().float().cpu(); b = b.detach().float()
    torch.testing.assert_close(a, b, rtol=rtol, atol=frac * max(1e-6, float(b.abs().max())), msg=lambda m: f"{name}: {m}")


def _template(net, ds):
    cameras, _, _ = net._cameras(2, DEV)
    net.angThred = cameras.angThreshold(0.5)
    verts, faces = net.discretizeSDF(RATIO, None, 0.0)
    assert 800 < verts.shape[0] < 5000
    net.TmpVs, net.Tmpfs = verts, faces
    net.TmpVs.requires_grad = True
    net.TmpOptimizer = torch.optim.SGD([net.TmpVs], lr=0.05, momentum=0.9)
    net.forward_time = 1                                     # the template is in place: no remesh inside forward()
    return cameras


def test_compute_tmp_pc_loss_vs_oracle():
    from selfreconcode_amd import mlp_engine
    net, ds, conf = _scene()
    cameras = _template(net, ds)
    sc = _oracle_scene(net, ds)
    fids = torch.tensor([3, 11], device=DEV); fo = fids.cpu()
    N = 2
    gt = ds.batch(fids)['mask']
    # ---- product
    poses, trans, d_cond, _ = ds.get_grad_parameters(fids, DEV)
    defconds = [d_cond, [poses, trans]]
    defTmpVs = net.deformer(net.TmpVs[None].expand(N, -1, 3), defconds, ratio=RATIO)
    masks = net._silhouette(defTmpVs, cameras, H, W, net.point_radius)
    radius = int(np.round(net.point_radius / 2. * float(min(H, W)) / 1.2))
    assert radius == 1
    mgt = torch.nn.functional.max_pool2d(gt, kernel_size=3, stride=1, padding=1)
    net.info = {'pc_loss': {}}
    V0 = net.TmpVs.detach().clone()
    out = net.computeTmpPcLoss(defTmpVs, defconds, masks, mgt, RATIO)
    # ---- oracle
    TmpVs_o = V0.cpu().clone().requires_grad_(True)
    opt_o = torch.optim.SGD([TmpVs_o], lr=0.05, momentum=0.9)
    defo = sc.deform(TmpVs_o[None].expand(N, -1, 3), sc.dcond[fo], sc.poses[fo], sc.trans[fo], None, RATIO)
    mo, _ = ito.ro.render_point_silhouette(defo, sc.cam['focal'], sc.cam['princ'], sc.cam['R'], sc.cam['T'], H, W, sc.point_radius, 50)
    close(masks, mo, 1e-4, 1e-4, "silhouette")
    info = {}
    outo = ito.pc_loss(sc, TmpVs_o, opt_o, defo, sc.dcond[fo], sc.poses[fo], sc.trans[fo], mo, torch.nn.functional.max_pool2d(gt.cpu(), 3, 1, 1), RATIO, info)
    close(net.info['pc_loss']['mask_loss'], info['mask_loss'], 1e-4, 1e-5, "mask_loss")
    close(net.info['pc_loss']['defconst_loss'], info['defconst_loss'], 1e-4, 1e-5, "defconst_loss")
    torch.testing.assert_close(net.info["pc_loss_sdf"].cpu(), info["pc_loss_sdf"], rtol=1e-4, atol=2e-6)          # mean |f| of vertices that sit ON the zero set: the value tolerance of f itself
    torch.testing.assert_close(out.detach().cpu(), outo.detach(), rtol=1e-4, atol=60 * 2e-6)
    # template SGD step: moved vertices (displacement compared, not the position)
    step, step_o = net.TmpVs.detach() - V0, TmpVs_o.detach() - V0.cpu()
    assert float(step_o.abs().max()) > 1e-7
    close(step, step_o, 1e-3, 2e-3, "template step")
    # gradients the INNER backward deposited for the outer Adam (network.py:686)
    mlp_engine.flush_param_grads()
    tr = net.deformer.defs[0]
    for n in ("lin0.weight", "lin2.weight", "lin4.weight", "lin4.bias", "lin1.bias"):
        close(dict(tr.named_parameters())[n].grad, sc.tr[n].grad, 1e-3, 2e-3, "deformer " + n)
    close(ds.conds[0].grad[fids], sc.dcond.grad[fo], 1e-3, 2e-3, "d_cond"); close(ds.poses.grad[fids], sc.poses.grad[fo], 1e-3, 2e-3, "poses")
    close(ds.trans.grad[fids], sc.trans.grad[fo], 1e-3, 2e-3, "trans")
    # backward of the |f(TmpVs)| term: the reference leaves it to the outer backward; here it is back-propagated where it is computed
    # (optim_network.EAGER_TEMPLATE_TERM: the returned term is then a value) -- the SDF has no other gradient at this point either way
    if out.requires_grad:
        for t in net.sdf.parameters():
            t.grad = None
        out.backward()
    mlp_engine.flush_param_grads(); outo.backward()
    for n in ("lin0.weight_v", "lin4.weight_g", "lin8.weight_v", "lin8.bias", "lin6.bias"):
        close(dict(net.sdf.named_parameters())[n].grad, sc.sdf[n].grad, 1e-3, 1e-3, "sdf " + n)


def test_whole_iteration_with_injected_randoms_vs_oracle():
    from selfreconcode_amd import mlp_engine
    mlp_engine.set_deferred_param_grads(True)                # the mode bench.py runs
    try:
        net, ds, conf = _scene()
        _template(net, ds)
        sc = _oracle_scene(net, ds)
        fids = torch.tensor([3, 11], device=DEV); fo = fids.cpu()
        N, SP = 2, 100
        datas = ds.batch(fids)
        big = 20000
        rand = {'ray_select': fx.det_tensor((big,), 41, 0.5) + 0.5, 'vert_select': fx.det_tensor((big,), 42, 0.5) + 0.5,
                'vert_select2': fx.det_tensor((big,), 43, 0.5) + 0.5, 'eik_local': fx.det_normal((big, 3), 44), 'eik_global': fx.det_tensor((big, 3), 45, 0.5) + 0.5,
                'regu_local': fx.det_normal((big, 3), 46)}
        V0 = net.TmpVs.detach().clone()
        dbg = {}
        loss = net(datas, SP, RATIO, fids, rand={k: v.to(DEV) for k, v in rand.items()}, debug=dbg)
        loss.backward()
        net.propagateTmpPsGrad(fids, RATIO)
        assert 120 < dbg['check'].numel() < 400 and int(dbg["check"].sum()) > 10, (dbg['check'].numel(), int(dbg['check'].sum()))
        # ---- oracle on the same template, data and draws; rays after the refiner are taken from the product (threshold flips)
        TmpVs_o = V0.cpu().clone().requires_grad_(True)
        opt_o = torch.optim.SGD([TmpVs_o], lr=0.05, momentum=0.9)
        do = {k: v.cpu() for k, v in datas.items()}
        F = ds.frame_num
        bf = lambda f, n: ((f - n // 2).clamp(min=0, max=F - n)).view(-1, 1) + torch.arange(n).view(1, n)
        tot, info, st = ito.forward(sc, TmpVs_o, net.Tmpfs.cpu(), opt_o, do, SP, RATIO, fo, rand, dctnull=net.dctnull.cpu(), batchframe=bf,
                                    inject={'initTmpPs': dbg['initTmpPs'].cpu(), 'check': dbg['check'].cpu()})
        # identical ray selection and seeds (mesh rasteriser + FindSurfacePs + Bernoulli draw)
        assert torch.equal(info['bi'], dbg['batch_inds'].cpu()) and torch.equal(info['rows'], dbg['row_inds'].cpu()) and torch.equal(info['cols'], dbg['col_inds'].cpu())
        close(dbg['seeds'], info['p0'], 1e-5, 1e-5, "seeds")
        i = net.info
        for k, v in (('mask_loss', i['pc_loss']['mask_loss']), ('defconst_loss', i['pc_loss']['defconst_loss']), ('pc_loss_sdf', i['pc_loss_sdf']),
                     ('grad_loss', i['grad_loss']), ('def_loss', i['def_loss']), ('dct_loss', i['dct_loss']), ('color_loss', i['color_loss']),
                     ('normal_loss', i['normal_loss'])):
            if k == 'pc_loss_sdf':                           # mean |f| of vertices that sit on the zero set: the value tolerance of f itself
                torch.testing.assert_close(v.cpu(), info[k], rtol=2e-4, atol=2e-6)
            else:
                close(v, info[k], 2e-4, 2e-4, k)
        close(loss, tot, 2e-4, 2e-4, "total loss")
        tot.backward()
        n_sys, n_ok = ito.propagate(sc, st, fo, RATIO)
        assert int(net.info['invInfo'][0]) == n_sys and abs(int(net.info['invInfo'][1]) - n_ok) <= 1
        close(net.TmpPs.grad, st['TmpPs'].grad, 1e-3, 2e-3, "dL/dTmpPs")
        for mod, sd, tag in ((net.sdf, sc.sdf, "sdf"), (net.deformer.defs[0], sc.tr, "deformer"), (net.netRender, sc.rnd, "render")):
            for n, p in mod.named_parameters():
                assert p.grad is not None, tag + " " + n
                close(p.grad, sd[n].grad, 2e-3, 3e-3, tag + " " + n)
        close(ds.poses.grad, sc.poses.grad, 2e-3, 3e-3, "poses"); close(ds.trans.grad[fids], sc.trans.grad[fo], 2e-3, 3e-3, "trans")
        close(ds.conds[0].grad[fids], sc.dcond.grad[fo], 2e-3, 3e-3, "d_cond")
        # camera: focal length, principal point and T are learnable in the shipped configuration (config.conf:10-15); their gradients come
        # from the silhouette projection (inner backward), the per-pixel rays (colour branch) and the implicit differentiation (:798-813)
        for key, okey in (('focal_length', 'focal'), ('princeple_points', 'princ'), ('world2cam_coord_trans', 'T')):
            assert ds.camera_params[key].requires_grad and ds.camera_params[key].grad is not None, key
            close(ds.camera_params[key].grad, sc.cam[okey].grad, 3e-3, 3e-3, "camera " + key)
        assert ds.conds[1].grad is None or float(ds.conds[1].grad.abs().max()) == 0.0     # rendcond[batch_inds] is passed and ignored (utils.py:171-172)
    finally:
        mlp_engine.set_deferred_param_grads(False)


def test_propagate_tmp_ps_grad_vs_the_references_own_run(golden):
    """a15 against the reference ITSELF: tests/golden/propagate.npz holds the gradients that the reference's
    OptimNetwork.propagateTmpPsGrad (model/network.py:702-814) deposited when run verbatim on CPU (oracle/gen_golden.py) -- SDF,
    deformation MLP, poses / translations / codes and the learnable focal length / principal point / T.  The product runs the same
    call (fused implicit solve, forward-mode Jacobian, deferred weight gradients on their own stream) on the same inputs."""
    import numpy as np
    from selfreconcode_amd import mlp_engine
    from selfreconcode_amd.model.network import getTmpSdf
    from selfreconcode_amd.model.Deformer import MLPTranslator, LBSkinner, CompositeDeformer
    from selfreconcode_amd.model.optim_network import OptimNetwork
    from selfreconcode_amd.utils import smpl_tmp_Apose
    g = golden("propagate")
    sdf = getTmpSdf(DEV, 6, 0.6, 256)
    sdf.load_state_dict(fx.det_params(fx.SDF_SPEC, 101), strict=True)
    tr = MLPTranslator(128, 6).to(DEV)
    tr.load_state_dict(fx.det_params(fx.DEF_SPEC, 202), strict=True)
    skin = LBSkinner(fx.synthetic_lbs_volume((7, 11, 9)), fx.LBS_BMIN, fx.LBS_BMAX, fx.synthetic_joints(), np.array(fx.SMPL_PARENTS),
                     init_pose=torch.from_numpy(smpl_tmp_Apose(1)), align_corners=False).to(DEV)
    ds = scene.Sequence(g["poses"].shape[0], int(g["HW"][0]), int(g["HW"][1]), DEV, tensors=g)
    net = OptimNetwork(sdf, CompositeDeformer([tr, skin]).to(DEV), None, None, None, conf=None)
    net.dataset = ds
    fids = g["fids"].long().to(DEV)
    net.batch_inds, net.col_inds, net.row_inds = g["bi"].long().to(DEV), g["cols"].long().to(DEV), g["rows"].long().to(DEV)
    net.TmpPs = g["p"].to(DEV).clone().requires_grad_(True)
    net.TmpPs.grad = g["glp"].to(DEV).clone()
    cameras, _, _ = net._cameras(3, torch.device(DEV))
    net.rays = cameras.view_rays(torch.stack([net.col_inds, net.row_inds, torch.ones_like(net.col_inds)], dim=-1).float())
    assert net.rays.requires_grad
    for deferred in (True, False):
        for t in list(sdf.parameters()) + list(tr.parameters()) + ds.learnable_weights():
            t.grad = None
        net.TmpPs.grad = g["glp"].to(DEV).clone()
        mlp_engine.set_deferred_param_grads(deferred)
        try:
            net.info = {}
            net.propagateTmpPsGrad(fids, RATIO)
        finally:
            mlp_engine.set_deferred_param_grads(False)
        assert int(net.info['invInfo'][0]) == int(g["inv_info"][0]) and abs(int(net.info['invInfo'][1]) - int(g["inv_info"][1])) <= 1
        sp, tp = dict(sdf.named_parameters()), dict(tr.named_parameters())
        tol = dict(rtol=3e-3, frac=3e-3)                               # float32 through (b^T b)^-1 on both sides (the CPU oracle meets the same fixture to 2e-3)
        close(ds.poses.grad, g["g_poses"], name="poses", **tol); close(ds.trans.grad, g["g_trans"], name="trans", **tol)
        close(ds.conds[0].grad, g["g_dcond"], name="dcond", **tol)
        close(ds.camera_params['focal_length'].grad, g["g_focal"], name="focal", **tol)
        close(ds.camera_params['princeple_points'].grad, g["g_princ"], name="princ", **tol)
        close(ds.camera_params['world2cam_coord_trans'].grad, g["g_T"], name="T", **tol)
        close(sp['lin0.weight_v'].grad[::37, ::5], g["g_sdf_v0"], name="sdf v0", **tol); close(sp['lin4.weight_g'].grad, g["g_sdf_g4"], name="sdf g4", **tol)
        close(sp['lin7.bias'].grad, g["g_sdf_b7"], name="sdf b7", **tol); close(sp['lin8.weight_v'].grad[:1, ::7], g["g_sdf_v8"], name="sdf v8", **tol)
        close(tp['lin0.weight'].grad[::41, ::9], g["g_tr_w0"], name="tr w0", **tol); close(tp['lin2.weight'].grad[::53, ::47], g["g_tr_w2"], name="tr w2", **tol)
        close(tp['lin4.bias'].grad, g["g_tr_b4"], name="tr b4", **tol); close(tp['lin4.weight'].grad[:, ::11], g["g_tr_w4"], name="tr w4", **tol)
        assert ds.conds[1].grad is None or float(ds.conds[1].grad.abs().max()) == 0.0


def test_whole_iteration_vs_the_references_own_run(golden):
    """The PRODUCT against the reference's own whole iteration (tests/golden/iteration.npz: OptimNetwork.forward + backward +
    propagateTmpPsGrad of the reference run verbatim on CPU with the pytorch3d renderers replaced by the restated ones, every random
    draw recorded -- oracle/gen_iteration_golden.py).  Same weights, data and draws: identical ray selection and seeds; the refiner's
    output against the reference's (flags flip on single ulps, so it is compared on its own and the reference's is used after it);
    every loss term, the total, the template SGD step, dL/dTmpPs and the gradients of the three networks, poses / translations /
    codes and the learnable focal length / principal point / T."""
    import _product_scene as ps
    from selfreconcode_amd.config import default_config
    from selfreconcode_amd.utils.FindSurfacePs import OptimizeSurfacePs
    g = golden("iteration")
    nets = sdf, tr, _, rn = ps.product_networks((7, 11, 9), DEV)
    ds = scene.Sequence(g["poses"].shape[0], int(g["HW"][0]), int(g["HW"][1]), DEV, tensors=g)
    net = ps.product_net(ds, nets, None, default_config().get_config('loss_coarse'), g["radius"], g["ang_thr"], g["V0"], g["faces"].long())
    net.dctnull = golden("misc")["dctnull"].to(DEV)
    fids = g["fids"].long().to(DEV)
    datas = {'img': g["img"].to(DEV), 'mask': g["mask"].to(DEV), 'normal': g["normal"].to(DEV)}
    rand = {k[5:]: v.to(DEV) for k, v in g.items() if k.startswith("rand_")}
    SP = int(g["SP"])

    # (1) the refiner on the reference's selected rays against the reference's refiner
    with torch.no_grad():
        poses, trans, d_cond, _ = [t.detach() for t in ds.get_grad_parameters(fids)]
        p1, ok = OptimizeSurfacePs(g["cam_pos"].to(DEV), g["sel_rays"].to(DEV), g["sel_p0"].to(DEV).clone(), g["sel_bi"].long().to(DEV), sdf, RATIO,
                                   net.deformer, [d_cond, [poses, trans]], dthreshold=5.e-5, athreshold=net.angThred, w1=3.05, w2=1., times=10)
    ref_ok = g["sel_check"].bool()
    assert float((ok.cpu() == ref_ok).float().mean()) > 0.95
    both = ok.cpu() & ref_ok
    assert int(both.sum()) > 50
    dev_p = (p1.cpu()[both] - g["sel_p1"][both]).abs().amax(1)           # (rays that zigzag towards a threshold amplify 1-ulp differences)
    assert float((dev_p < 2e-5).float().mean()) > 0.9 and float(dev_p.max()) < 5e-4, (float((dev_p < 2e-5).float().mean()), float(dev_p.max()))

    # (2) the whole iteration with the reference's draws and the reference's refiner output
    rand['refined'] = (g["sel_p1"], ref_ok)
    with ps.deferred_param_grads():
        dbg = {}
        loss = net(datas, SP, RATIO, fids, rand=rand, debug=dbg)
        assert torch.equal(dbg['batch_inds'].cpu(), g["sel_bi"].long()) and dbg['batch_inds'].numel() == int(g["ray_info"][0])
        close(dbg['seeds'], g["sel_p0"], 1e-5, 1e-5, "seeds"); close(dbg['rays'], g["sel_rays"], 1e-5, 1e-5, "rays")
        i = net.info
        for k, v in (('mask_loss', i['pc_loss']['mask_loss']), ('defconst_loss', i['pc_loss']['defconst_loss']), ('grad_loss', i['grad_loss']),
                     ('def_loss', i['def_loss']), ('dct_loss', i['dct_loss']), ('color_loss', i['color_loss']), ('normal_loss', i['normal_loss']),
                     ('offset_loss', i['offset_loss'])):
            close(v, g["L_" + k], 3e-4, 3e-4, k)
        torch.testing.assert_close(i['pc_loss_sdf'].cpu().float(), g["L_pc_loss_sdf"].float(), rtol=2e-3, atol=2e-6)
        close(loss, g["loss"], 3e-4, 3e-4, "total loss")
        assert torch.equal(net.batch_inds.cpu(), g["bi"].long()) and torch.equal(net.row_inds.cpu(), g["rows"].long()) and torch.equal(net.col_inds.cpu(), g["cols"].long())
        step, step_ref = net.TmpVs.detach().cpu() - g["V0"], g["V1"] - g["V0"]
        close(step, step_ref, 2e-3, 3e-3, "template step")
        loss.backward()
        close(net.TmpPs.grad, g["g_TmpPs"], 2e-3, 3e-3, "dL/dTmpPs")
        net.propagateTmpPsGrad(fids, RATIO)
    assert int(net.info['invInfo'][0]) == int(g["inv_info"][0]) and abs(int(net.info['invInfo'][1]) - int(g["inv_info"][1])) <= 1
    sp, tp, rp = dict(sdf.named_parameters()), dict(tr.named_parameters()), dict(rn.named_parameters())
    tol = dict(rtol=4e-3, frac=4e-3)
    bad = []

    def cmp(a, b, rtol=1e-3, frac=1e-3, name=""):        # collect every mismatch of the gradient block before failing
        try:
            close(a, b, rtol, frac, name)
        except AssertionError as e:
            bad.append(name + ": " + str(e).split("Greatest absolute difference:")[1].split("\n")[0].strip() + " max " + str(float(b.abs().max())))
    cmp(ds.poses.grad, g["g_poses"], name="poses", **tol); cmp(ds.trans.grad, g["g_trans"], name="trans", **tol); cmp(ds.conds[0].grad, g["g_dcond"], name="dcond", **tol)
    cmp(ds.camera_params['focal_length'].grad, g["g_focal"], name="focal", **tol); cmp(ds.camera_params['princeple_points'].grad, g["g_princ"], name="princ", **tol)
    cmp(ds.camera_params['world2cam_coord_trans'].grad, g["g_T"], name="T", **tol)
    cmp(sp['lin0.weight_v'].grad[::37, ::5], g["g_sdf_v0"], name="sdf v0", **tol); cmp(sp['lin4.weight_g'].grad, g["g_sdf_g4"], name="sdf g4", **tol)
    cmp(sp['lin7.bias'].grad, g["g_sdf_b7"], name="sdf b7", **tol); cmp(sp['lin8.weight_v'].grad[::16, ::7], g["g_sdf_v8"], name="sdf v8", **tol)
    cmp(tp['lin0.weight'].grad[::41, ::9], g["g_tr_w0"], name="tr w0", **tol); cmp(tp['lin2.weight'].grad[::53, ::47], g["g_tr_w2"], name="tr w2", **tol)
    cmp(tp['lin4.bias'].grad, g["g_tr_b4"], name="tr b4", **tol); cmp(tp['lin4.weight'].grad[:, ::11], g["g_tr_w4"], name="tr w4", **tol)
    cmp(rp['lin0.weight_v'].grad[::31, ::13], g["g_rn_v0"], name="render v0", **tol); cmp(rp['lin2.weight_g'].grad, g["g_rn_g2"], name="render g2", **tol)
    cmp(rp['lin4.bias'].grad, g["g_rn_b4"], name="render b4", **tol)
    assert ds.conds[1].grad is None or float(ds.conds[1].grad.abs().max()) == 0.0
    assert not bad, bad
