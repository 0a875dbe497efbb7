"""TEST INFRASTRUCTURE ONLY -- K = 32 consecutive training iterations of the REFERENCE AT THE SIZE BASELINE.json configs[1] IS QUOTED ON,
with one remesh on the shipped coarse grid, run verbatim on CPU and frozen into tests/golden/trajectory_full.npz (build container only:
needs /root/reference; ~25 s per iteration on 8 cores):

    python oracle/gen_trajectory_full_golden.py [--k K] [--twin]

`--twin` (run with `--k 14`): the SAME reference run with every template coordinate one float32 ulp away, up to and including the remesh
iteration and the one after it; its per-iteration mask errors are merged into trajectory_full.npz as `twin_maskE_it` / `twin_remesh_nV` /
`twin_L_total`.  How far the reference's own twin lands from the reference is the noise floor of everything that follows the remesh (the
SDF's zero set after REMESH_AT Adam steps on an L1 term is decided by float32 rounding): the GPU test takes its bound from it.

This is the quality pin SURVEY.md's north_star asks for ("matching silhouette IoU after equal iterations"): the reference's only
quantitative quality metric is the mask error 1 - IoU of the rasterised deformed template against the ground-truth mask
(infer.py:172-181, computed model/network.py:322-324).  The loop is train.py:147-170 -- `optimizer.zero_grad(); loss = optNet(...);
loss.backward(); optNet.propagateTmpPsGrad(...); optimizer.step()` -- with Adam(lr 1e-4: the rate config.conf runs the coarse stage at)
over the dataset's learnable tensors and the three networks, the template's SGD inside forward, on the scene of
oracle/gen_fullsize_golden.py's coarse stage: 540 x 540, 3 frames x 2048 rays per iteration, the real 65 x 225 x 129 skinning-weight
volume, a template of 84 968 vertices, loss_coarse.  At the call with index REMESH_AT `forward_time % remesh_intersect == 0`
(network.py:463-478): the reference's own Seg3dLossless (MCAcc/seg3d_lossless.py, CPU) on the coarse pyramid of train.py:29-37
(15 x 21 x 9 ... 225 x 321 x 129) + the reference's own marching-cubes kernels (oracle/_ref/libmc_ref_fma.so) behind `MCGpu.mc_gpu`.
Harness as oracle/gen_iteration_golden.py (pytorch3d renderers -> oracle/raster_oracle.py, CUDA extensions / torch_scatter -> their
pinned restatements).  Draw c of iteration k is det_tensor / det_normal with seed DRAW_BASE + 16 k + c, so the product regenerates them.

Stored per iteration: every loss term and the total, rayInfo (rays selected, rays the refiner accepted), the template's vertex count,
and -- the quality metric -- the mask error 1 - IoU of EVERY frame of the batch (from the fragments the mesh rasteriser stand-in hands
`forward`: the same silhouette `infer` rasterises); at the remesh the vertex / face counts and a strided vertex sample; at the end maskE
of `infer` on EVAL_FRAMES and parameter digests.
"""
import os
import sys
import time
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import gen_iteration_golden as gi  # noqa: E402
from oracle import gen_fullsize_golden as gf  # noqa: E402
from oracle import scene  # noqa: E402
from oracle import ref_scene as rs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
K, REMESH_AT = 32, 12
NUDGE_BELOW = 4e-5
LR = 1e-4
EVAL_FRAMES = [2, 11, 19, 30]
RES_COARSE = [(15, 21, 9), (29, 41, 17), (57, 81, 33), (113, 161, 65), (225, 321, 129)]       # train.py:29-37
RES_FINE = [(21, 27, 15), (41, 53, 29), (81, 105, 57), (161, 209, 113), (321, 417, 225)]        # train.py:45-51
# `--stage fine`: the stage 189 of the reference's 201 epochs run in -- 1 frame x 6144 rays per iteration (config.conf:43-48,113), loss_fine, a
# 173 402-vertex template, remesh on 321 x 417 x 225, Adam at 1e-4 * 0.333^3 (the MultiStepLR value of epochs 80-129) -> trajectory_full_fine.npz
STAGE = {"coarse": dict(N=3, res=RES_COARSE, lr=1e-4, radius=0.006, base=29000, remesh=30, name="trajectory_full.npz"),
         "fine": dict(N=1, res=RES_FINE, lr=1e-4 * 0.333 ** 3, radius=0.0041, base=39000, remesh=120, name="trajectory_full_fine.npz")}


# `--scene consistent` (round 6): a scene the optimisation can CONVERGE on.  The noise fixture above shows that the product follows the
# reference through chaos (its mask error goes UP at the remesh); this one shows the quality metric FALLING on both sides at the same
# rate: the ground-truth mask of a frame is the silhouette -- the reference's own deformer, the mesh-rasteriser restatement -- of the
# initial template scaled by CONS_SCALE, so the template's SGD step on the mask loss has a silhouette it can reach; colour and normal
# targets are smooth functions of the pixel inside that mask (`scene.consistent_observation`, one function for both sides), white /
# zero outside as `infer` renders them.  Eight frames cycle through the batch so that every frame comes back every few iterations.
CONS_FRAMES = [2, 7, 11, 19, 21, 26, 30, 35]
CONS_SCALE = 1.05


def main():
    kk = K
    if "--k" in sys.argv:
        kk = int(sys.argv[sys.argv.index("--k") + 1])
    twin = "--twin" in sys.argv
    stage = sys.argv[sys.argv.index("--stage") + 1] if "--stage" in sys.argv else "coarse"
    cfg = STAGE[stage]
    CONSISTENT = "--scene" in sys.argv and sys.argv[sys.argv.index("--scene") + 1] == "consistent"
    if CONSISTENT:
        assert stage == "coarse"
        cfg = dict(cfg, base=49000, name="trajectory_full_consistent.npz")
    noray = "--no-ray-terms" in sys.argv        # (diagnostics) colour / normal weights 0: no ray branch, no implicit-gradient pass -> trajectory_full_noray.npz
    cover_only = "--cover" in sys.argv          # re-run up to the remesh and merge the rasterised silhouettes of that iteration into the fixture (bit-packed)
    torch.set_num_threads(os.cpu_count())
    t_start = time.perf_counter()
    f64 = "--f64" in sys.argv                   # (diagnostics) the same modules evaluated in double on the same float32-representable inputs; prints only
    net, ds, _, _, q, V0, faces = gf.build(stage, dtype=torch.float64 if f64 else torch.float32)
    # The coarse-stage fixture's template sits ON the zero set of the initial SDF by construction (one-iteration parity wants converging
    # rays), with 4e-3 offsets that leave ~0.1 % of the vertices at |f| < 3e-5 -- and a handful below the 3e-7 to which any float32
    # evaluation of f is reproducible.  The L1 template term's gradient is sign(f) per vertex and Adam's first steps are sign steps, so
    # those few coin tosses set the whole trajectory on another path (measured: ten flipped vertices at k = 0 -> 4 % in mean |f| after ONE
    # step, 0.02 in maskE after the remesh, with the reference's own one-ulp twin 0.003 away).  A trajectory fixture must not hang on
    # them: vertices with |f| < NUDGE_BELOW are moved 3e-4 of their radius outwards (their indices are stored; both sides apply the same
    # float32 multiply), after which min |f| over the template is > 1e-5.
    with torch.no_grad():
        f0 = torch.cat([net.sdf(part, 1.0)[:, 0] for part in torch.split(net.TmpVs.detach(), 20000)])
        nudge_idx = torch.nonzero(f0.abs() < NUDGE_BELOW).view(-1)
        net.TmpVs[nudge_idx] = net.TmpVs[nudge_idx] * 1.0003
        f1 = torch.cat([net.sdf(part, 1.0)[:, 0] for part in torch.split(net.TmpVs.detach(), 20000)])
        print(f"template: {nudge_idx.numel()} of {f0.numel()} vertices with |f| < {NUDGE_BELOW} nudged; min |f| before {float(f0.abs().min()):.2e}, after {float(f1.abs().min()):.2e}", flush=True)
        assert float(f1.abs().min()) > 1e-5
    if twin:
        with torch.no_grad():
            net.TmpVs.mul_(1.0 + 1.2e-7)
    if noray:
        net.conf = gi.DictConf(dict(gi.LOSS_COARSE, color_weight=0., normal_weight=-0.1))
    H = W = 540
    F = ds.frame_num
    N = cfg["N"]
    SPX = 2048                                   # (the fine stage's loss_fine carries sample_pix_num = 6144, which overrides it: network.py:520)
    net.engine = rs.seg3d_engine(cfg["res"])
    remeshed = {}

    def on_remesh(V, Fc, seconds):
        remeshed.update(V=V, F=Fc)
        print(f"    marching cubes (reference kernels, host build): {seconds:.1f} s, V = {V.shape[0]}, F = {Fc.shape[0]}", flush=True)
    rs.install_mc_stand_ins(on_remesh)
    net.forward_time, net.remesh_intersect = cfg["remesh"] - REMESH_AT, cfg["remesh"]          # one remesh in the window: at the call with index REMESH_AT
    optimizer = scene.adam_over(ds, net, cfg["lr"])
    gtm1 = scene.elliptic_mask(H, W)[None]
    cons_masks, obs_cache = {}, {}
    frames_of = lambda k: scene.frames_full(k, F, N, CONS_FRAMES if CONSISTENT else None)
    if CONSISTENT:
        with torch.no_grad():
            cf = torch.tensor(CONS_FRAMES)
            poses, trans, dcond, _ = ds.get_grad_parameters(cf, 'cpu')
            tgt = net.deformer((net.TmpVs.detach() * CONS_SCALE)[None].expand(len(CONS_FRAMES), -1, 3), [dcond, [poses, trans]], ratio=scene.ratio_of(0))
            cover = rs.silhouettes(tgt, ds, faces, H, W)
            for i, f in enumerate(CONS_FRAMES):
                cons_masks[f] = cover[i]
            print("consistent scene: target silhouettes of", CONS_FRAMES, "cover", [int(m.sum()) for m in cons_masks.values()], "pixels", flush=True)

    out = dict(q=q.view(-1), nudge_idx=nudge_idx.to(torch.int32), HW=np.array([H, W]), SP=np.array(SPX), K=np.array(kk), remesh_at=np.array(REMESH_AT), remesh_intersect=np.array(cfg["remesh"]), frame_num=np.array(F), lr=np.array(cfg["lr"]), frames_per_iteration=np.array(N),
               radius=np.array(cfg["radius"]), ang_thr=np.array(net.angThred), res=np.array(cfg["res"]), eval_frames=np.array(EVAL_FRAMES), lbs_shape=np.array([65, 225, 129]),
               n_cube=np.array(gf.STAGES[stage]["n_cube"]), draw_base=np.array(cfg["base"]))
    rows, ray_counts, draw_shapes, vcount, maskE_it, seconds = [], [], [], [], [], []
    for k in range(kk):
        t0 = time.perf_counter()
        fids = torch.tensor(frames_of(k))
        draws = scene.KeyedDraws(cfg["base"], k)
        with rs.patched(draws):
            optimizer.zero_grad()
            obs = scene.consistent_batch([cons_masks[int(f)] for f in fids]) if CONSISTENT else scene.noise_observations(fids, H, W, cache=obs_cache)
            if f64:
                obs = {k_: v_.double() for k_, v_ in obs.items()}
                torch.Tensor.float, real_float = (lambda self, *a, **kw: self.to(torch.float64)), torch.Tensor.float
            try:
                loss = net(obs, SPX, scene.ratio_of(k), fids)
            finally:
                if f64:
                    torch.Tensor.float = real_float
            loss.backward()
            net.propagateTmpPsGrad(fids, scene.ratio_of(k))
            optimizer.step()
        info = net.info
        rows.append(scene.loss_row(info, loss))
        ray_counts.append([int(info['rayInfo'][0]), int(info['rayInfo'][1])])
        draw_shapes.append(draws.shape_rows(pad_to=6))
        vcount.append(net.TmpVs.shape[0])
        cover = (net.maskRender.last_p2f[..., 0] >= 0).float()
        maskE_it.append(scene.mask_error(cover, obs['mask'].float() if CONSISTENT else gtm1.expand(N, H, W)).tolist())
        if k == REMESH_AT:
            out["cover_at_remesh"] = np.packbits(cover.numpy().astype(np.uint8))
        if 'V' in remeshed and "remesh_V" not in out:
            out["remesh_V"], out["remesh_nV"], out["remesh_nF"], out["remesh_k"] = remeshed['V'][::11].clone(), np.array(remeshed['V'].shape[0]), np.array(remeshed['F'].shape[0]), np.array(k)
        seconds.append(time.perf_counter() - t0)
        print(k, frames_of(k), "loss %.6f" % float(loss), "rays", info['rayInfo'], "V", net.TmpVs.shape[0], "maskE", np.round(maskE_it[-1], 4).tolist(),
              "%.1f s" % seconds[-1], flush=True)
    if f64:
        print("float64 evaluation: total loss per iteration", [round(r['total'], 6) for r in rows], "pc_loss_sdf", [round(r['pc_loss_sdf'], 6) for r in rows])
        return
    if kk > REMESH_AT:
        assert "remesh_V" in out and int(out["remesh_k"]) == REMESH_AT
    # ---- the end state: maskE of `infer` (network.py:306-324) on EVAL_FRAMES, parameter digests
    ef = CONS_FRAMES[:4] if CONSISTENT else EVAL_FRAMES
    maskE = rs.end_state(net, ds, net.deformer, ef, scene.ratio_of(kk), H, W, torch.stack([cons_masks[f] for f in ef]) if CONSISTENT else gtm1.expand(len(ef), H, W))
    out.update(maskE=maskE, maskE_it=np.array(maskE_it), ray_counts=np.array(ray_counts), draw_shapes=np.array(draw_shapes), vcount=np.array(vcount),
               seconds_per_iteration=np.array(seconds), cores=np.array(os.cpu_count()),
               **rs.loss_curves(rows))
    rs.write_digests(out, net.sdf, net.deformer.defs[0], net.netRender)
    out["final_cam"] = torch.cat([ds.focal.detach(), ds.princ.detach(), ds.T.detach()])
    if CONSISTENT:
        out["cons_frames"] = np.array(CONS_FRAMES)
        out["cons_scale"] = np.array(CONS_SCALE)
        out["cons_masks"] = np.stack([np.packbits(cons_masks[f].numpy().astype(np.uint8)) for f in CONS_FRAMES])
        out["eval_frames"] = np.array(ef)
    conv = rs.to_numpy(out)
    if cover_only:
        main = dict(np.load(os.path.join(OUT, cfg["name"])))
        # (the reference on CPU is not bit-reproducible run to run -- multi-threaded reductions: after ~9 iterations a re-run accepts one ray
        # more or less; the silhouettes agree to a few pixels)
        dev = float(np.abs(main["maskE_it"][:kk] - conv["maskE_it"]).max())
        print("re-run against the fixture: max |maskE difference| %.5f" % dev)
        assert dev < 5e-3, "the re-run did not reproduce the fixture"
        main["cover_at_remesh"] = conv["cover_at_remesh"]
        np.savez_compressed(os.path.join(OUT, cfg["name"]), **main)
        print("merged cover_at_remesh into", cfg["name"])
        return
    if twin:                                                             # merged into the main fixture
        main = dict(np.load(os.path.join(OUT, cfg["name"])))
        main.update(twin_maskE_it=conv["maskE_it"], twin_remesh_nV=conv.get("remesh_nV", np.array(-1)), twin_L_total=conv["L_total"], twin_ray_counts=conv["ray_counts"])
        np.savez_compressed(os.path.join(OUT, cfg["name"]), **main)
        print("merged the twin into " + cfg["name"] + ": max |maskE - twin| before the remesh %.5f, from it on %.4f; remesh vertices %d against %d" % (
            np.abs(main["maskE_it"][:REMESH_AT] - conv["maskE_it"][:REMESH_AT]).max(), np.abs(main["maskE_it"][REMESH_AT:kk] - conv["maskE_it"][REMESH_AT:kk]).max(),
            int(main["remesh_nV"]), int(conv.get("remesh_nV", -1))))
        return
    name = "trajectory_full_noray.npz" if noray else (cfg["name"] if kk == K else f"trajectory_full_{stage}_k{kk}.npz")
    np.savez_compressed(os.path.join(OUT, name), **conv)
    rc = np.array(ray_counts, dtype=np.float64)
    print("wrote", name, os.path.getsize(os.path.join(OUT, name)), "bytes; total %.0f s; maskE" % (time.perf_counter() - t_start), maskE.tolist())
    print("converged fraction per 8 iterations:", [round(float(rc[a:a + 8, 1].sum() / rc[a:a + 8, 0].sum()), 3) for a in range(0, kk, 8)])


if __name__ == "__main__":
    main()
