"""NumPy restatement of the fuser bank's feature path (include/ndtgpu.h "the fuser bank's feature path", steps 2-6):
ndt_feature_fuser_hmt.cpp:252-334 (feature pose, consistency gate, FLIRT cell pairs in front of the odometry cells) and :497-502 (the
points moved to the new pose).  Sequential and plain, with the scalar loops of tests/test_gpu_fuser_bank.py (mm, rigid_inv, euler012):
every product is rounded before it is added, in the order of csrc/ndt_pose.h and csrc/ndt_fuserfeat.h, so records and cells can be
compared bit for bit.  Poses are 4x4 row-major NumPy arrays here."""
import math

import numpy as np

from test_gpu_fuser_bank import euler012, mm, rigid_inv

MAX_CELLS, ODOM_CELLS = 64, 40
OK = 0
IJ = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def T_of_record(r):
    """the 4x4 of ndtgpu_featbank_match_device's T16: built from (c, s, x, y), no trigonometry"""
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1], T[0, 3], T[1, 3] = r["c"], -r["s"], r["s"], r["c"], r["x"], r["y"]
    return T


def gate(prm, fprm, Tnow, Tmotion, ransac):
    """steps 2, 3 and the counts of step 5.  prm / fprm: objects with the fields of ndtgpu_fuser_params / ndtgpu_fuser_feat_params;
    ransac: a record (mapping with status, n_inliers, c, s, x, y) or None: RANSAC not run"""
    sensor = np.array(list(prm.sensor_pose)).reshape(4, 4).T
    n_odom = ODOM_CELLS if (prm.use_odom and not prm.fusion2d) else 0
    rec = dict(ransac_run=0, consistent=0, n_feat_cells=0, n_odom_cells=n_odom, truncated=0, Tfeat=np.zeros((4, 4)))
    if ransac is None or not fprm.use_feat:
        return rec
    rec["ransac_run"] = 1
    Tfeat = mm(T_of_record(ransac), rigid_inv(sensor))
    rec["Tfeat"] = Tfeat
    consistent = int(ransac["status"]) == OK and int(ransac["n_inliers"]) > 0
    if consistent and prm.check_consistency:
        diff = mm(rigid_inv(mm(Tnow, Tmotion)), Tfeat)
        e = euler012(diff)
        dt = math.sqrt(diff[0, 3] * diff[0, 3] + diff[1, 3] * diff[1, 3] + diff[2, 3] * diff[2, 3])
        dr = math.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
        if dt > prm.max_translation_norm / 10. or dr > prm.max_rotation_norm / 4.:
            consistent = False
    rec["consistent"] = int(consistent)
    if fprm.use_feat and consistent and not prm.fusion2d:
        room = MAX_CELLS - n_odom
        rec["n_feat_cells"] = min(int(ransac["n_inliers"]), room)
        rec["truncated"] = int(int(ransac["n_inliers"]) > room)
    return rec


def pseudo(T, mean, cov):
    """pseudoTransformNDTMap on one Gaussian: mean' = T mean, cov' = R cov R^T, the loops of ndtgpu_fuser_prepare"""
    m = [float(T[a, 0]) * mean[0] + float(T[a, 1]) * mean[1] + float(T[a, 2]) * mean[2] + float(T[a, 3]) for a in range(3)]
    RC = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += float(T[i, k]) * float(cov[k, j])
            RC[i, j] = s
    out = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += float(RC[i, k]) * float(T[j, k])
            out[i, j] = s
    return m, out


def half(mean, cov):
    return [mean[0], mean[1], mean[2]] + [float(cov[i, j]) for i, j in IJ]


def cell_pair(prm, fprm, Tnow, cur3, prev3, prev_as_is):
    sensor = np.array(list(prm.sensor_pose)).reshape(4, 4).T
    cell = []
    for side, p in enumerate((cur3, prev3)):
        m = [float(p[0]), float(p[1]), 0.0]
        C = np.diag([float(v) for v in fprm.feat_cov])
        if side == 0 or not prev_as_is:
            m, C = pseudo(sensor, m, C)
            m, C = pseudo(Tnow, m, C)
        cell += half(m, C)
    return cell


def odom_cell(pp, last):
    """one of the 40 odometry cell pairs from ndtgpu_fuser_prepare's values (tests/test_gpu_fuser_bank.py feat_of)"""
    return (list(pp["feat_src_mean"]) + list(pp["feat_cov_plain"] if last else pp["feat_cov_rotated"]) + list(pp["feat_tgt_mean"])
            + list(pp["feat_cov_rotated"]))


def prepare(prm, fprm, Tnow, Tmotion, pp, ransac, corr, cur_pos, prev_pos, prev_moved=False):
    """ndtgpu_fuser_feat_prepare -> (record dict, cells [n_cells, 18]); pp: ndtgpu_fuser_prepare's values for (Tnow, Tmotion)"""
    rec = gate(prm, fprm, Tnow, Tmotion, ransac)
    as_is = bool(fprm.prev_in_map_frame) and bool(prev_moved)
    cells = [cell_pair(prm, fprm, Tnow, cur_pos[int(corr[l][0])], prev_pos[int(corr[l][1])], as_is) for l in range(rec["n_feat_cells"])]
    cells += [odom_cell(pp, l == rec["n_odom_cells"] - 1) for l in range(rec["n_odom_cells"])]
    return rec, np.array(cells, dtype=np.float64).reshape(-1, 18)


def move(T, pos):
    """step 6: P = pose2d(x, y, theta) as a 4x4, M = T P, (M[0,3], M[1,3], eulerAngles(0,1,2)(M)[2])"""
    out = np.zeros((len(pos), 3))
    for i, p in enumerate(pos):
        c, s = math.cos(p[2]), math.sin(p[2])
        P = np.eye(4)
        P[0, 0], P[0, 1], P[1, 0], P[1, 1], P[0, 3], P[1, 3] = c, -s, s, c, p[0], p[1]
        M = mm(T, P)
        out[i] = [M[0, 3], M[1, 3], euler012(M)[2]]
    return out


def hand_made_pair(K, seed, pose=(0.3, -0.2, 0.05), desc_len=48, noise=1e-3):
    """The fixture of the feature tests: K points on a jittered grid (0.8 m spacing, +-0.1 m jitter), descriptors uniform in
    (0.1, 1) and equal in both sets; prev = the points under a known rigid pose plus `noise` m on the positions (exact copies can
    reach a score of exactly 0).  At the default RANSAC parameters K = 20, 24, 30 end OK with K inliers and corr (i, i); K = 19
    ends TOO_FEW (n_c * 0.1 < 2).  -> (cur_pos [K, 3], prev_pos [K, 3], desc [K, desc_len], the pose as a 4x4)"""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(K)))
    g = np.array([[i % side, i // side] for i in range(K)], dtype=np.float64) * 0.8
    cur = np.zeros((K, 3))
    cur[:, :2] = g + rng.uniform(-0.1, 0.1, size=(K, 2))
    cur[:, 2] = rng.uniform(-1.0, 1.0, size=K)
    desc = rng.uniform(0.1, 1.0, size=(K, desc_len))
    x, y, th = pose
    c, s = math.cos(th), math.sin(th)
    prev = np.zeros((K, 3))
    prev[:, 0] = c * cur[:, 0] - s * cur[:, 1] + x
    prev[:, 1] = s * cur[:, 0] + c * cur[:, 1] + y
    prev[:, :2] += rng.uniform(-noise, noise, size=(K, 2))
    prev[:, 2] = cur[:, 2] + th
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1], T[0, 3], T[1, 3] = c, -s, s, c, x, y
    return cur, prev, desc, T
