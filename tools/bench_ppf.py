"""Times of the pose proposals (utils/ppf.py, csrc/ppf.hip) on an L-shaped prism: the table build (the pair launch, the
sort and the CSR), the normals of the scene, the vote launch, the cluster launch, and beside them the ICP launch that
refines the candidates they ride along with.  HIP events around the Python wrappers, warm-up calls first, min / median / max in microseconds.  The scenes are surface samples of the mesh
that face the camera under sampled poses, with the faces' normals.  Also printed: how many samples have a proposal
within the method's two thresholds of the truth, and, from the bucket lengths of sample 0, the share of lane steps that
would do work if every lane walked its own bucket, and that do with a wave's items dealt to its lanes, as the kernel
does (profiles/notes_ppf.md).

    python tools/bench_ppf.py [--quick]        # --quick: B = 8, N = 256, M = 256 only, few repetitions (for a profiler)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_verify_reference as V
import ppf_reference as P
from cloudaae_amd.utils import icp, mesh_models as mm, pose_score, ppf
from cloudaae_amd.utils import sample_pose_in_frustum as spf

quick = "--quick" in sys.argv
torch.cuda.set_device(0)
dev = torch.device("cuda:0")
lv, lt = V.l_prism()
mesh = [((lv.astype(np.float64) * 1.5).astype(np.float32), lt)]


def timed(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return dict(min_us=round(min(ts), 1), median_us=round(float(np.median(ts)), 1), max_us=round(max(ts), 1), n=n)


def scenes(B, N, seed):
    """B clouds of N surface samples that face the camera under sampled poses, their normals, and the poses."""
    s = mm.sample_meshes(mesh, 6 * N, seed=seed, return_normals=True, device=dev)
    pts, nrm = s['xyzrgb'][0, :, :3].double().cpu().numpy(), s['normal'][0].cpu().numpy()
    poses = spf.sample_poses(B, 7, 0, device=dev)
    gt = pose_score.pose_matrix(poses['axisangle'], poses['translation']).cpu().numpy()
    xyz, normals = np.zeros((B, N, 3), np.float32), np.zeros((B, N, 3))
    for b in range(B):
        p = pts @ gt[b, :3, :3].T + gt[b, :3, 3]
        n = nrm @ gt[b, :3, :3].T
        seen = np.nonzero((n * -p).sum(axis=1) > 0.0)[0][:N]
        assert len(seen) == N
        xyz[b], normals[b] = p[seen], n[seen]
    return torch.from_numpy(xyz).to(dev), torch.from_numpy(normals).to(dev), gt


def lane_shares(models, xyz, normals, ref_step):
    """Sample 0: (useful lane steps / lane steps) with one bucket per lane, and with a wave's items dealt to its lanes."""
    x, n = xyz[0].cpu().numpy(), normals[0].cpu().numpy()
    bs = models.bucket_start[0].cpu().numpy().astype(np.int64)
    work = own = flat = 0
    for r in range(0, len(x), ref_step):
        key, d = P.pair_key(x[r], n[r], x, n, float(models.dist_step[0]), models.n_dist, models.n_angle, models.tables[0])
        ok = (key >= 0) & P.direction(P.frame(n[r]), d)[0]
        ok[r] = False
        length = np.where(ok, bs[np.maximum(key, 0) + 1] - bs[np.maximum(key, 0)], 0)
        for w in range(0, len(x), 64):
            c = length[w:w + 64]
            work += int(c.sum())
            own += 64 * int(c.max())
            flat += 64 * -(-int(c.sum()) // 64)
    return dict(entries_walked=work, own_bucket_share=round(work / max(own, 1), 3), dealt_share=round(work / max(flat, 1), 3),
                mean_bucket=round(float(work) / max(len(range(0, len(x), ref_step)) * len(x), 1), 1))


res = {}
obj = mm.models_from_meshes(mesh, num_point=2048, device=dev)                  # the ICP's object model
for M in ((256,) if quick else (256, 512)):
    reps = dict(n=5, warm=2) if quick else dict(n=10, warm=2)
    models = ppf.PPFModels.from_meshes(mesh, num_point=M, device=dev)
    pts, nrm = models.xyz.clone(), models.normals.clone()
    res['table_build_M%d' % M] = dict(timed(lambda: ppf.PPFModels.from_points([pts], [nrm], models.diameters[:1], device=dev), **reps),
                                      entries=models.n_entries, keys_in_use=int((models.bucket_start[0].diff() > 0).sum()),
                                      longest_bucket=int(models.bucket_start[0].diff().max()))
    tt2, rot_bound = P.thresholds(models.diameters)
    for B in ((8,) if quick else (8, 32)):
        for N in ((256,) if quick else (256, 1024)):
            tag = 'B%d_N%d_M%d' % (B, N, M)
            xyz, normals, gt = scenes(B, N, 11)
            mask = torch.ones((B, N), dtype=torch.uint8, device=dev)
            cls = torch.zeros(B, dtype=torch.int64, device=dev)
            reps = dict(n=5, warm=2) if quick else dict(n=20, warm=3)
            res['vote_%s' % tag] = timed(lambda: ppf.vote(models, xyz, normals, mask, cls), **reps)
            v = ppf.vote(models, xyz, normals, mask, cls)
            res['cluster_%s' % tag] = timed(lambda: ppf.cluster(models, v['votes'].view(B, -1), v['pose'].view(B, -1, 4, 4), cls), **reps)
            res['scene_normals_%s' % tag] = timed(lambda: ppf.scene_normals(xyz, 0.02), **reps)
            r = ppf.propose_poses(models, xyz, normals, mask, cls, top=4)
            pose, ok = r['pose'].cpu().numpy(), r['valid'].cpu().numpy()
            hit = [any(ok[b, t] and (lambda e: e[0] ** 2 <= tt2[0] and e[1] >= rot_bound)(P.pose_errors(pose[b, t], gt[b]))
                       for t in range(4)) for b in range(B)]
            first = [bool(ok[b, 0]) and (lambda e: e[0] ** 2 <= tt2[0] and e[1] >= rot_bound)(P.pose_errors(pose[b, 0], gt[b]))
                     for b in range(B)]
            res['found_%s' % tag] = dict(best_of_4_within_thresholds=int(sum(hit)), first_within_thresholds=int(sum(first)), of=B)
            res['lanes_%s' % tag] = lane_shares(models, xyz, normals, 5)
            if N == 256:
                # the ICP launch of the evaluation: 2048 model points onto the N scene points, 4 flips + 4 proposals per sample
                K = 8
                rot = icp.to_float32(r['rot_axag']).repeat(1, 2, 1).view(B * K, 3).contiguous()
                tr = r['trans'].repeat(1, 2, 1).view(B * K, 3).contiguous()
                o, sc = obj.repeat(B * K, 1, 1), xyz.repeat_interleave(K, dim=0).contiguous()
                res['icp_%d_candidates_%s' % (B * K, tag)] = timed(lambda: icp.refine_pose_icp(o, sc, rot, tr), n=5, warm=1)
print(json.dumps(res, indent=1))
