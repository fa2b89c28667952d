"""The optimiser's index structure of a local-BA window restated for the tests of tc2li_host_ba_structure and of the device-built structure:
ba_build_structure (tc2li-slam_amd/csrc/ba_structure.hpp:69-229, line numbers below are that file's) for the sparse path -- at most 24 free
poses, which is every covisibility window.  Written from the text with plain loops and lists: this is the yardstick, not an implementation."""
LEAN_SLOTS, SLICE_LANDMARKS, GROUP_LEAN, BLOCKS_MAX_FREE, LEAN_MAX_FREE = 128, 64, 8, 21, 24   # ba_device.hpp:23, :26, :39; ba_structure.hpp:131


class Invalid(Exception):
    pass


def _ranges(nf, pref, room):                                                           # ba_device.hpp:27-31, :40-43
    for rd, ro in pref:
        if rd * nf + ro * (nf * (nf - 1) // 2) + nf <= room:
            return rd, ro
    return pref[-1]


def structure(fixed, n_points, edge_point, edge_pose, extra_used=None):
    n_poses, n_edges = len(fixed), len(edge_point)
    used = [0] * n_poses
    for e in range(n_edges):                                                           # :77-83
        if not (0 <= edge_pose[e] < n_poses and 0 <= edge_point[e] < n_points):
            raise Invalid("edge %d out of range" % e)
        used[edge_pose[e]] = 1
    if extra_used is not None:                                                         # :84
        used = [1 if (u or x) else 0 for u, x in zip(used, extra_used)]
    pose_var, n_free = [-1] * n_poses, 0
    for k in range(n_poses):                                                           # :85
        if not fixed[k] and used[k]:
            pose_var[k], n_free = n_free, n_free + 1
    assert n_free <= LEAN_MAX_FREE, "the restatement covers the sparse path"
    by_point = [[] for _ in range(n_points)]                                           # :89-104: edges of a point in edge order
    by_pose = [[] for _ in range(n_free)]
    for e in range(n_edges):
        by_point[edge_point[e]].append(e)
    for l in range(n_points):                                                          # :90-93
        if not by_point[l]:
            raise Invalid("point %d has no edge" % l)
    pt_off = [0]
    for l in range(n_points):
        pt_off.append(pt_off[-1] + len(by_point[l]))
    pt_edges = [e for l in range(n_points) for e in by_point[l]]
    fl_off, fl_pose, fl_lm, fl_place, fl_edge, w_slot, slice_off, dups = [], [], [], [], [], [-1] * n_edges, [0], []
    slice_lms = 0
    for l in range(n_points):                                                          # :144-164, landmarks in index order (no dense window)
        begin, seen = len(fl_pose), {}
        for e in by_point[l]:
            i = pose_var[edge_pose[e]]
            if i < 0:                                                                  # :148
                continue
            if i in seen:                                                              # :155: the later edge of a pair gets no slot
                dups.append((i, e, seen[i]))
                continue
            seen[i] = len(fl_pose)
            w_slot[e] = len(fl_pose)                                                   # :157
            fl_pose.append(i); fl_lm.append(l); fl_edge.append(e); fl_place.append(None)
        at = len(fl_pose)
        fl_off += [begin, at]                                                          # :159
        if at == begin:                                                                # :160
            continue
        if slice_lms == SLICE_LANDMARKS or at - slice_off[-1] > LEAN_SLOTS:            # :161
            slice_off.append(begin)
            slice_lms = 0
        fl_place[begin:at] = [slice_lms] * (at - begin)                                # :162
        slice_lms += 1
    n_slots = len(fl_pose)
    if n_slots > slice_off[-1]:                                                        # :165
        slice_off.append(n_slots)
    for e in range(n_edges):                                                           # :94 / :176-181: the edges that have a slot, by pose
        if w_slot[e] >= 0:
            by_pose[pose_var[edge_pose[e]]].append(e)
    pv_off = [0]
    for i in range(n_free):
        pv_off.append(pv_off[-1] + len(by_pose[i]))
    dups.sort(key=lambda d: (d[0], d[1]))                                              # :174
    dup_off = [sum(1 for d in dups if d[0] < i) for i in range(n_free + 1)]
    n_blocks = (n_slots + 255) // 256                                                  # :184
    blk_off, blk_rows = [], []
    for b in range(max(n_blocks, 1)):                                                  # :189-197: a stable sort of the block's slots by pose
        rows = sorted(range(256 * b, min(n_slots, 256 * b + 256)), key=lambda s: fl_pose[s]) if b < n_blocks else []
        blk_off += [sum(1 for s in rows if fl_pose[s] < i) for i in range(n_free + 1)]
        blk_rows += [s - 256 * b for s in rows] + [0] * (256 - len(rows))
    grp_k0, grp_l0 = [0], [0]
    for l in range(n_points):                                                          # :201-204
        if pt_off[l + 1] - pt_off[l] > 256:
            raise Invalid("point %d has more than 256 edges" % l)
        if pt_off[l + 1] - grp_k0[-1] > 256:
            grp_k0.append(pt_off[l]); grp_l0.append(l)
    grp_k0.append(n_edges); grp_l0.append(n_points)                                    # :205
    n_groups = len(grp_k0) - 1
    max_group_landmarks = max(grp_l0[g + 1] - grp_l0[g] for g in range(n_groups))
    if max_group_landmarks > 256:                                                      # :210
        raise Invalid("more than 256 landmarks in a group")
    n_schur_slices = len(slice_off) - 1
    wide = n_free > BLOCKS_MAX_FREE                                                    # :41, :61
    rd, ro = _ranges(n_free, [(4, 1), (3, 1), (2, 1), (1, 1)], 512) if wide else \
        _ranges(n_free, [(5, 2), (4, 2), (3, 2), (2, 2), (3, 1), (2, 1), (1, 1)], 256)
    return dict(n_free=n_free, n_slots=n_slots, n_free_pose_edges=n_slots + len(dups), n_dups=len(dups), n_blocks=n_blocks, n_groups=n_groups,
                max_group_landmarks=max_group_landmarks, np=6 * n_free, np_pad=(6 * n_free + 1 + 15) // 16 * 16,                # :43-46
                n_schur_slices=n_schur_slices, n_slices=(n_schur_slices + GROUP_LEAN - 1) // GROUP_LEAN, k_per_slice=0,         # :49-51
                schur_group=GROUP_LEAN, sparse=1, schur_rd=rd, schur_ro=ro,
                pose_var=pose_var, pt_off=pt_off, pt_edges=pt_edges, pv_off=pv_off, pv_edges=[e for i in range(n_free) for e in by_pose[i]],
                fl_off=fl_off, fl_pose=fl_pose, fl_lm=fl_lm, fl_place=fl_place, fl_edge=fl_edge, w_slot=w_slot, slice_off=slice_off,
                dup_off=dup_off, dup_edge=[d[1] for d in dups], dup_slot=[d[2] for d in dups], blk_off=blk_off, blk_rows=blk_rows,
                grp_k0=grp_k0, grp_l0=grp_l0, chunk_mask=[])
