"""TEST INFRASTRUCTURE ONLY -- K = 64 consecutive training iterations of the REFERENCE with FOUR remeshes and the coarse -> medium
stage switch, run verbatim on CPU and frozen into tests/golden/trajectory_long.npz (build container only: needs /root/reference):
    python oracle/gen_trajectory_long_golden.py

The loop is train.py:147-170 on the miniature sequence of oracle/gen_trajectory_golden.py (same networks, dataset stand-in, renderer
stand-ins, draws keyed by (iteration, call order), Adam lr 1e-4 = the rate config.conf runs its first ten epochs at):
  * coarse stage (loss_coarse, 3 frames per iteration, point radius 0.045, remesh every 12 calls: at k = 6, 18, 30);
  * at k = 24 -- an epoch boundary in train.py:148-152 -- `utils.set_hierarchical_config(conf, 'medium', ...)` (utils/utils.py:237-255):
    2 frames per iteration from now on, a new Seg3dLossless engine on the medium pyramid, `next_conf` / `next_train_conf` pending;
  * the pending configuration is adopted by `update_hierarchical_config` inside forward at the NEXT remesh (network.py:172-205,464):
    k = 30; from there loss_medium, radius 0.035, remesh every 20 calls (k = 50).
`update_hierarchical_config` of the reference builds pytorch3d renderer objects; here its ten lines run with the harness's renderer
stand-ins (same assignments: conf, forward_time = 0, point radius, remesh interval, sdfShrinkRadius = 0, pending configs cleared).

Stored per iteration: every loss term and the total, rayInfo (rays selected, rays the refiner accepted), template vertex count, the stage;
per remesh: iteration, vertex / face count, a strided vertex sample; at the end maskE of `infer` on four frames (network.py:322-324)
and parameter digests.  This is the reference's counterpart of bench.py's lr-1e-4 regime: the fraction of rays its own refiner accepts
while Adam runs at 1e-4, on a sequence both sides can run.
"""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import gen_iteration_golden as gi  # noqa: E402
from oracle import gen_fullsize_golden as gf  # noqa: E402
from oracle import fixtures as fx  # noqa: E402
from oracle import scene  # noqa: E402
from oracle import ref_scene as rs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
K = 64
F, H, W, SP = 36, 64, 64, 300
FIRST_REMESH, SWITCH_AT = 6, 24
STAGE = {"coarse": dict(N=3, radius=0.045, remesh=12, res=[(15, 21, 9), (29, 41, 17), (57, 81, 33)], loss=gi.LOSS_COARSE),
         "medium": dict(N=2, radius=0.035, remesh=20, res=[(19, 25, 13), (37, 49, 25), (73, 97, 49)], loss=gf.LOSS_MEDIUM)}
LBS_SHAPE = (17, 57, 33)
LR = 1e-4
DRAW_BASE = 19000
EVAL_FRAMES = [2, 11, 19, 30]


def main():
    torch.set_num_threads(os.cpu_count())
    nets = sdf, tr, comp, rn = rs.reference_networks(LBS_SHAPE)
    ds = scene.Sequence(F, H, W)
    remeshes = []
    rs.install_mc_stand_ins(lambda V, Fc, seconds: remeshes.append((V, Fc.shape[0])))
    dirs, faces = fx.icosphere(3)
    q = rs.radii_on_zero_set(sdf, dirs)
    coarse, medium = STAGE["coarse"], STAGE["medium"]
    net = rs.reference_net(ds, nets, scene.template_from_q(dirs, q), faces, coarse["loss"], H, W, coarse["radius"], remesh_intersect=coarse["remesh"],
                           first_remesh=FIRST_REMESH, engine=rs.seg3d_engine(coarse["res"]))
    stage_now = {"name": "coarse"}

    def update_hierarchical_config(device):                             # network.py:172-205 with the harness's renderer stand-ins
        if net.next_conf is not None:
            net.conf = net.next_conf
            net.forward_time = 0
            net.pcRender = gi.PcRender(H, W, net.next_train_conf['radius'])
            net.pcRender.rasterizer.cameras = net.maskRender.rasterizer.cameras          # `cameras=rasterizer.cameras` (network.py:186)
            net.remesh_intersect = net.next_train_conf['remesh']
            net.sdfShrinkRadius = 0.0
            net.next_conf = None
            net.next_train_conf = None
            stage_now["name"] = "medium"
    net.update_hierarchical_config = update_hierarchical_config
    optimizer = scene.adam_over(ds, net, LR)
    out = dict(q=q.view(-1), HW=np.array([H, W]), SP=np.array(SP), K=np.array(K), frame_num=np.array(F), lr=np.array(LR), first_remesh=np.array(FIRST_REMESH),
               switch_at=np.array(SWITCH_AT), ang_thr=np.array(net.angThred), eval_frames=np.array(EVAL_FRAMES), lbs_shape=np.array(LBS_SHAPE),
               **{f"{s}_{k}": np.array(v) for s, d in STAGE.items() for k, v in d.items() if k != "loss"})
    rows, ray_counts, draw_shapes, vcount, stage_of, remesh_iters = [], [], [], [], [], []
    nbatch = coarse["N"]
    for k in range(K):
        if k == SWITCH_AT:                                              # train.py:148-152 -> utils.set_hierarchical_config (utils/utils.py:237-255)
            nbatch = medium["N"]
            net.next_conf = gi.DictConf(medium["loss"])
            net.next_train_conf = {"radius": medium["radius"], "remesh": medium["remesh"]}
            net.engine = rs.seg3d_engine(medium["res"])
        fids = torch.tensor(scene.frames_64(k, F, nbatch))
        draws = scene.KeyedDraws(DRAW_BASE, k)
        nrem = len(remeshes)
        with rs.patched(draws):
            optimizer.zero_grad()
            loss = net(scene.noise_observations(fids, H, W), SP, scene.ratio_of(k), fids)
            loss.backward()
            net.propagateTmpPsGrad(fids, scene.ratio_of(k))
            optimizer.step()
        info = net.info
        rows.append(scene.loss_row(info, loss))
        ray_counts.append([int(info['rayInfo'][0]), int(info['rayInfo'][1])])
        draw_shapes.append(draws.shape_rows(pad_to=6))
        vcount.append(net.TmpVs.shape[0]); stage_of.append(0 if stage_now["name"] == "coarse" else 1)
        if len(remeshes) > nrem:
            remesh_iters.append(k)
            out[f"remesh{len(remesh_iters) - 1}_V"] = remeshes[-1][0][::7].clone()
        print(k, stage_now["name"], scene.frames_64(k, F, nbatch), "loss %.6f" % float(loss), info['rayInfo'], "V", net.TmpVs.shape[0], flush=True)
    maskE = rs.end_state(net, ds, comp, EVAL_FRAMES, scene.ratio_of(K), H, W, scene.elliptic_mask(H, W)[None].expand(len(EVAL_FRAMES), H, W))
    out.update(maskE=maskE, ray_counts=np.array(ray_counts), draw_shapes=np.array(draw_shapes), vcount=np.array(vcount), stage_of=np.array(stage_of),
               remesh_iters=np.array(remesh_iters), remesh_V=np.array([r[0].shape[0] for r in remeshes]), remesh_F=np.array([r[1] for r in remeshes]),
               **rs.loss_curves(rows))
    rs.write_digests(out, sdf, tr, rn)
    np.savez_compressed(os.path.join(OUT, "trajectory_long.npz"), **rs.to_numpy(out))
    print("wrote trajectory_long.npz", os.path.getsize(os.path.join(OUT, "trajectory_long.npz")), "bytes; remeshes at", remesh_iters, "maskE", maskE.tolist())
    rc = np.array(ray_counts, dtype=np.float64)
    print("converged fraction per 16 iterations:", [round(float(rc[a:a + 16, 1].sum() / rc[a:a + 16, 0].sum()), 3) for a in range(0, K, 16)])


if __name__ == "__main__":
    main()
