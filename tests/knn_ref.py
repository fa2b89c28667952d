"""Brute-force reference of the LiDAR 5-NN search: numpy float32 with the kernel's expression
(qx-mx)*(qx-mx) + (qy-my)*(qy-my) + (qz-mz)*(qz-mz), one rounded operation at a time, ordered by (distance, x)
like PointType_CMP with the x tie-break of the search.  No index structure, so nothing a grid can get wrong."""
import numpy as np

f32 = np.float32


def sqdist(map_points, q):
    """Squared distances (float32) of one query (x, y, z) to every map point."""
    dx, dy, dz = f32(q[0]) - map_points["x"], f32(q[1]) - map_points["y"], f32(q[2]) - map_points["z"]
    assert dx.dtype == np.float32
    return (dx * dx + dy * dy) + dz * dz


def knn5(map_points, queries):
    """-> (sqdist [n, 5], index [n, 5], nfound [n], gap [n]): the five smallest squared distances in (distance, x) order, the
    indices into map_points (-1 and distance 0 in empty slots), and the difference between the 6th and the 5th distance (inf
    where the map has fewer than 6 points)."""
    n, m = len(queries), len(map_points)
    d5, idx = np.zeros((n, 5), f32), np.full((n, 5), -1, np.int64)
    nfound, gap = np.full(n, min(m, 5), np.int32), np.full(n, np.inf)
    for i in range(n):
        d = sqdist(map_points, (queries["x"][i], queries["y"][i], queries["z"][i]))
        k = min(m, 6)
        cand = np.argpartition(d, k - 1)[:k] if m > k else np.arange(m)
        cand = np.flatnonzero(d <= d[cand].max()) if m else cand  # everything tied with the k-th as well
        order = cand[np.lexsort((map_points["x"][cand], d[cand]))]
        top = order[:5]
        d5[i, :len(top)], idx[i, :len(top)] = d[top], top
        if len(order) > 5:
            gap[i] = float(d[order[5]]) - float(d[order[4]])
    return d5, idx, nfound, gap
