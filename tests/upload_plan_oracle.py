"""An independent statement of what a graph upload plans on the host (visfs_amd/csrc/ba_plan.hpp): the summary of the observations and
the index structure of the reduced camera matrix S, written from the field documentation of DeviceGraph (visfs_amd/csrc/ba_device.hpp)
with brute-force loops, sets and sorting — no inclusion sums, no counting passes, no shared code with the C++.

`plan(g, d)`: g holds the graph (pose_fixed, point_fixed, obs_pose, obs_point, odo_from, odo_to, n_laser, laser_pose), d the decisions
of the upload (solver, batch_member, throughput, index_blocks, the switches, the kernels' answers); returns a dict of integer lists and
scalars under the names tests/cpp/plan_driver.cpp prints, or {"status": code, "msg": text} for a refusal."""
import numpy as np

LIN_CHUNK, SCH_CHUNK, RUN_GROUP, RUN_MAX_W, RUN_MAX_TILES, RUN_TILE, SM_MAX_N6 = 256, 64, 8, 64, 416, 21, 64
ERR_UNSUPPORTED = 7
INT_MAX = 0x7fffffff


def band_lds_bytes(npf, B, rows):
    """The stand-in tests/cpp/plan_driver.cpp answers with (the real one lives with the kernels)."""
    return 100000 * npf + 1000 * B + rows


def summary(g):
    fixed = np.asarray(g["pose_fixed"]).astype(bool)
    pfixed = np.asarray(g["point_fixed"]).astype(bool)
    free_pose = [i for i in range(len(fixed)) if not fixed[i]]
    pose_free = [free_pose.index(i) if not fixed[i] else -1 for i in range(len(fixed))]
    npf, nl = len(free_pose), len(pfixed)
    obs = list(zip(g["obs_point"], g["obs_pose"]))
    per_pose = [sum(1 for _, p in obs if p == i) for i in free_pose]
    pcount = np.zeros((npf, npf), np.int64)
    pairs = 0
    for l in range(nl):
        if pfixed[l]:
            continue
        seen = sorted(pose_free[p] for q, p in obs if q == l and not fixed[p])
        pairs += len(seen) * (len(seen) + 1) // 2
        for i, a in enumerate(seen):
            for b in seen[i:]:
                pcount[a, b] += 1
    grp = []
    for g0 in range(0, (nl + RUN_GROUP - 1) // RUN_GROUP + 1):
        poses = [p for l, p in obs if g0 * RUN_GROUP <= l < (g0 + 1) * RUN_GROUP]
        grp += [len(poses), min(poses) if poses else INT_MAX, max(poses) if poses else -1]
    return dict(pose_free=pose_free, free_pose=free_pose, cnt=[0] + list(np.cumsum(per_pose)), pcount=pcount, pairs_seen=pairs,
                n_edges_ok=sum(1 for l, p in obs if not (fixed[p] and pfixed[l])), grp=grp)


def summary_fast(g):
    """The same summary for the one large case (vectorised; checked against `summary` on the small graphs by the test)."""
    fixed = np.asarray(g["pose_fixed"]).astype(bool)
    pfixed = np.asarray(g["point_fixed"]).astype(bool)
    op, ol = np.asarray(g["obs_pose"], np.int64), np.asarray(g["obs_point"], np.int64)
    free_pose = np.flatnonzero(~fixed)
    pose_free = np.full(len(fixed), -1)
    pose_free[free_pose] = np.arange(len(free_pose))
    npf, nl = len(free_pose), len(pfixed)
    a = pose_free[op]
    member = np.zeros((nl, npf), np.int64)
    member[ol[a >= 0], a[a >= 0]] = 1
    member[pfixed] = 0
    pcount = np.triu(member.T @ member)
    c = member.sum(1)
    ng = (nl + RUN_GROUP - 1) // RUN_GROUP + 1
    gi = ol // RUN_GROUP
    gcnt = np.bincount(gi, minlength=ng)
    lo = np.full(ng, INT_MAX); hi = np.full(ng, -1)
    np.minimum.at(lo, gi, op); np.maximum.at(hi, gi, op)
    return dict(pose_free=list(pose_free), free_pose=list(free_pose), cnt=[0] + list(np.cumsum(np.bincount(a[a >= 0], minlength=npf))),
                pcount=pcount, pairs_seen=int((c * (c + 1) // 2).sum()), n_edges_ok=int((~(fixed[op] & pfixed[ol])).sum()),
                grp=list(np.stack([gcnt, lo, hi], 1).ravel()))


def plan(g, d, s=None):
    s = dict(s or summary(g))
    if d.get("pairs_seen", -1) >= 0: s["pairs_seen"] = d["pairs_seen"]          # synthetic (the refusal of a pair list beyond 2^31 - 1)
    fixed = np.asarray(g["pose_fixed"]).astype(bool)
    pose_free, free_pose, cnt, pcount = s["pose_free"], s["free_pose"], s["cnt"], s["pcount"]
    npc, nl, no, npf = len(fixed), len(g["point_fixed"]), len(g["obs_pose"]), len(free_pose)
    edges = list(zip(g["odo_from"], g["odo_to"]))
    ne = len(edges)
    nz = g["n_laser"] if g["n_laser"] > 0 and not fixed[g["laser_pose"]] else 0
    sw = lambda k, dflt=0: d.get(k, dflt)
    out = dict(s, status=0, Npf=npf, n_pose_obs=cnt[npf])
    out["pcount"] = list(np.asarray(pcount).ravel())

    # pose-major chunks: the observations of a free pose, cut every LIN_CHUNK
    chunks = [(a, k) for a in range(npf) for k in range(cnt[a], cnt[a + 1], LIN_CHUNK)]
    out["chunk_pose"] = [a for a, _ in chunks]
    out["chunk_ptr"] = [k for _, k in chunks] + [cnt[npf]]
    out["pose_chunk_ptr"] = [sum(1 for a, _ in chunks if a < q) for q in range(npf + 1)]
    out["n_chunks"] = len(chunks)

    # odometry incidence: edge * 2 + role, in edge order; the laser edges' pseudo edge 2 Ne last
    inc = [[] for _ in range(npf)]
    for e, (i, j) in enumerate(edges):
        if not fixed[i]: inc[pose_free[i]].append(2 * e)
        if not fixed[j]: inc[pose_free[j]].append(2 * e + 1)
    if nz: inc[pose_free[g["laser_pose"]]].append(2 * ne)
    out["pose_odo"] = [c for lst in inc for c in lst]
    out["pose_odo_ptr"] = [0] + list(np.cumsum([len(lst) for lst in inc]).astype(int))

    # stored blocks: the diagonal, every (a, b) with a common free landmark, every odometry edge between two free poses
    if s["pairs_seen"] > INT_MAX:
        return dict(status=ERR_UNSUPPORTED, msg="window too large (pair list)")
    blocks = {(a, a) for a in range(npf)} | {(int(a), int(b)) for a, b in np.argwhere(np.triu(np.asarray(pcount)) > 0)}
    blocks |= {tuple(sorted((pose_free[i], pose_free[j]))) for i, j in edges if not fixed[i] and not fixed[j]}
    blocks = sorted(blocks)
    n_blk = len(blocks)
    bid = {ab: b for b, ab in enumerate(blocks)}
    blk_ptr = [0] + list(np.cumsum([int(pcount[a][b]) for a, b in blocks]).astype(int))
    if blk_ptr[-1] > INT_MAX:
        return dict(status=ERR_UNSUPPORTED, msg="window too large (pair list)")
    out.update(blk_i=[a for a, _ in blocks], blk_j=[b for _, b in blocks], blk_ptr=blk_ptr, n_blk=n_blk, npairs=blk_ptr[-1],
               blk_of=[bid.get((a, b), -1) for a in range(npf) for b in range(npf)])
    bo = [[] for _ in blocks]
    for e, (i, j) in enumerate(edges):
        if fixed[i] or fixed[j]: continue
        a, b = pose_free[i], pose_free[j]
        bo[bid[(min(a, b), max(a, b))]].append(2 * e + (1 if a > b else 0))
    out["blk_odo"] = [c for lst in bo for c in lst]
    blk_odo_ptr = out["blk_odo_ptr"] = [0] + list(np.cumsum([len(lst) for lst in bo]).astype(int))

    # adjacency of the block rows of the symmetric S, by ascending column
    rows = [[] for _ in range(npf)]
    for b, (i, j) in enumerate(blocks):
        rows[i].append((j, 2 * b))
        if i != j: rows[j].append((i, 2 * b + 1))
    rows = [sorted(r) for r in rows]
    row_ptr = out["row_ptr"] = [0] + list(np.cumsum([len(r) for r in rows]).astype(int))
    out["row_col"] = [c for r in rows for c, _ in r]
    out["row_blk"] = [k for r in rows for _, k in r]
    max_row = out["max_row"] = out["cu_max_row"] = max([len(r) for r in rows], default=0)

    # the run plan of k_schur_runs
    run = run_plan(s["grp"], pose_free, bid, npc, nl, no, npf, d)
    out.update({"run_" + k: v for k, v in run.items()})
    run_path = run["n"] > 0

    # Schur chunks and the descriptors
    n64 = sum(-(-(blk_ptr[b + 1] - blk_ptr[b]) // SCH_CHUNK) for b in range(n_blk))
    passes = 2 if (not sw("batch_member") and 1024 <= n64 <= 6144) else 1
    if 1 <= sw("sch_passes") <= 8: passes = sw("sch_passes")
    sch_chunk = out["sch_chunk"] = SCH_CHUNK * passes
    sch = [] if run_path else [(b, k) for b in range(n_blk) for k in range(blk_ptr[b], blk_ptr[b + 1], sch_chunk)]
    out["sch_blk"] = [b for b, _ in sch]
    out["n_sch"] = len(sch)
    bcp = out["blk_chunk_ptr"] = [sum(1 for b, _ in sch if b < q) for q in range(n_blk + 1)]
    out["sch_desc"] = [v for b, k in sch for v in (k, min(k + sch_chunk, blk_ptr[b + 1]), free_pose[blocks[b][0]], free_pose[blocks[b][1]])]
    pcp = out["pose_chunk_ptr"]
    blk_desc, fin_exp = [], []
    for b, (i, j) in enumerate(blocks):
        lo, hi = (out["pose_odo_ptr"][i], out["pose_odo_ptr"][i + 1]) if i == j else (blk_odo_ptr[b], blk_odo_ptr[b + 1])
        x, y = bcp[b], bcp[b + 1]
        if run_path:
            nr = run["last"][b] - run["first"][b] + 1 if run["last"][b] >= 0 else 0
            x, y = (run["first"][b] if nr else 0) | nr << 20, free_pose[i] | free_pose[j] << 16
        blk_desc += [x, y, lo, hi, i, j, pcp[i], pcp[i + 1]]
        fin_exp.append((bcp[b + 1] - bcp[b]) | ((pcp[i + 1] - pcp[i]) << 16 if i == j else 0))
    out.update(blk_desc=blk_desc, fin_exp=fin_exp, diag_blk=[bid[(a, a)] for a in range(npf)])
    out.update(sizeof_sch_desc=max(len(sch), 1), sizeof_blk_desc=2 * max(n_blk, 1), sizeof_blk_slot=max(n_blk, 1))

    # the PCG forms
    solver = sw("solver")
    if solver == 2 and npf > 1024:
        return dict(status=ERR_UNSUPPORTED, msg="Optimizer/Solver=2 (PCG) supports at most 1024 free poses; use the direct solver")
    rpw = out["pcg_rpw"] = -(-npf // 256) if npf > 256 else 1
    lds = (12 * npf + 32 + 32 * rpw + (6 * npf if npf > 256 else 0)) * 8 + 8 * max_row * rpw + 16
    srow = out["lds_srow"] = 1 if lds + 288 * max_row * rpw <= 150 * 1024 else 0
    lds = out["pcg_lds"] = lds + srow * 288 * max_row * rpw
    if solver == 2 and lds > 160 * 1024:
        return dict(status=ERR_UNSUPPORTED, msg="reduced camera system too large for the persistent PCG (LDS); use the direct solver")
    pcg1 = out["pcg1"] = int(solver == 2 and 1 <= npf <= 64 and sw("pcg1", 1) != 0)
    code = np.full((npf, npf), -1, np.int64)
    for r in range(npf):
        for c, k in rows[r]: code[r, c] = k
    out["pcg1_code"] = list(code.ravel()) if pcg1 else []
    want_cu = sw("pcg_cu", -1) == 1 if sw("pcg_cu", -1) >= 0 else bool(sw("throughput"))
    pcg_cu = out["pcg_cu"] = int(solver == 2 and sw("pcg_cu_fits", 1) != 0 and 6 * npf > 64 and want_cu)
    out["cu_T"] = -(-6 * npf // 64) * 64
    slot = []
    for b, (i, j) in enumerate(blocks):
        ki = [c for c, _ in rows[i]].index(j)
        kj = [c for c, _ in rows[j]].index(i) if i != j else 255
        slot.append((ki | kj << 8) if pcg_cu else (255 | 255 << 8))
    out["blk_slot"] = slot

    # the band of the direct solver
    out.update(band_B=-1, band_rows=0, band_lds=0, band_code=[])
    if npf >= 1:
        B = max(j - i for i, j in blocks)
        rows_a = sw("band_plan_rows") or npf
        lds_a = sw("band_plan_lds", 4096)
        if sw("band", 1) != 0 and sw("band_plan_ok", 1) != 0:
            q = sw("band_rows")
            if B + 3 <= q < rows_a: rows_a, lds_a = q, band_lds_bytes(npf, B, q)
            bc = np.full((npf, B + 1), -1, np.int64)
            for b, (i, j) in enumerate(blocks): bc[j, j - i] = b
            out.update(band_B=B, band_rows=rows_a, band_lds=lds_a, band_code=list(bc.ravel()))
        elif sw("band", 1) != 0:
            out.update(band_rows=rows_a, band_lds=lds_a)          # (what the predicate left behind; band_B = -1 says it is not used)

    # launch shapes
    group = 4
    while group < 64 and group < (no / nl if nl > 0 else 1.0): group *= 2
    if nl >= 1024 and group > 8: group = 8
    if sw("group") in (4, 8, 16, 32, 64): group = sw("group")
    n_lin_a = max(1, -(-nl // (256 // group)))
    out.update(group=group, n_lin_a=n_lin_a, n_parts=max(n_lin_a + 1, (no + 255) // 256 + 1), chol_np=max(32, -(-6 * npf // 32) * 32),
               small_fits=int(npf >= 1 and 6 * npf <= SM_MAX_N6), n_hist=max(sw("index_blocks", 1), 1) * max(npf, 1))
    return out


def run_plan(grp, pose_free, bid, npc, nl, no, npf, d):
    """k_schur_runs: a workgroup owns LR x M consecutive landmarks (a run); its blocks are those of its pose span [lo, lo + W)."""
    none = dict(LR=0, M=1, n=0, cap=0, wmax=0, lds=0, total=0, desc=[], first=[], last=[], k0=[])
    ng = (nl + RUN_GROUP - 1) // RUN_GROUP
    gcnt, glo, ghi = grp[0::3], grp[1::3], grp[2::3]
    if not (d.get("schur_runs") and npf >= 1 and no > 0 and nl > 0 and 6 * npf > SM_MAX_N6 and npc < 65536):
        return none
    cap_of = lambda LR: max(sum(gcnt[q:min(ng, q + LR // RUN_GROUP)]) for q in range(0, ng, LR // RUN_GROUP))
    fits = [(limit, LR) for limit in (176, RUN_MAX_TILES) for LR in (64, 32, 16, 8) if cap_of(LR) <= limit]
    if not fits:
        return none
    LR = fits[0][1]
    if d.get("run_lr", 0) in (8, 16, 32, 64) and d["run_lr"] < LR: LR = d["run_lr"]
    M = max(1, 32 // LR)
    while -(-nl // (LR * M)) > 1024 and M < 16: M *= 2
    if 1 <= d.get("run_m", 0) <= 16: M = d["run_m"]
    per = LR * M
    n = -(-nl // per)
    desc, total, wmax, nbmax = [], 0, 0, 0
    spans = []
    for r in range(n):
        qs = [q for q in range(r * per // RUN_GROUP, min(ng, (r + 1) * per // RUN_GROUP)) if gcnt[q] > 0]
        lo, hi = (min(glo[q] for q in qs), max(ghi[q] for q in qs)) if qs else (0, -1)
        W = hi - lo + 1
        if W > RUN_MAX_W:
            return none
        spans.append(range(lo, lo + W))
        desc += [lo, W, total, 0]
        total += W * (W + 1) // 2
        wmax, nbmax = max(wmax, W), max(nbmax, W * (W + 1) // 2)
    first, last = [INT_MAX] * len(bid), [-1] * len(bid)
    for (a, b), k in bid.items():
        mine = [r for r, sp in enumerate(spans) if any(pose_free[p] == a for p in sp) and any(pose_free[p] == b for p in sp)]
        if mine: first[k], last[k] = mine[0], mine[-1]
        if mine and mine[-1] - mine[0] + 1 > 4095: return none
    lds = ((max(cap_of(LR), -(-256 * 14 // RUN_TILE)) * RUN_TILE + 9 * LR + 9 * wmax) * 8 + ((LR * wmax + 3) & ~3) * 2 + nbmax * 2 + 15) & ~15
    gl = LR // RUN_GROUP
    k0 = [sum(gcnt[:min(ng, sb * gl)]) for sb in range(n * M + 1)]
    return dict(LR=LR, M=M, n=n, cap=cap_of(LR), wmax=wmax, lds=lds, total=total, desc=desc, first=first, last=last, k0=k0)
