"""Sequential restatement of the outline tracing of csrc/contours.hip (ops.trace_class_regions): numpy and plain Python,
no GPU and no project code.  It follows the rules one edge at a time, the way a border follower would.

region / sizes: int [n, h, w] as unet_label_class_regions makes them (region = 1 + the smallest linear index of the
pixel's 8-connected class region, sizes = its pixel count, both 0 on background).  A pixel is a member of a region iff it
carries that region's value; everything outside the frame is a non-member.  Regions below min_pixels have no edges.

A directed crack edge is (pixel p, direction d), d = 0 E (+x), 1 S (+y), 2 W, 3 N.  It exists when p is a member and its
neighbour in direction r = (d + 1) % 4 is not: the side of p that faces r, travelled in direction d.  Its id within the
image is 4 (y w + x) + d.  The successor of (p, d) is the first that applies of: (p + d + r, r) if p + d + r is a member
(turn right), (p + d, d) if p + d is a member (straight), (p, (d + 3) % 4) (turn left).  The edges fall into loops; a
loop's leader is its smallest id.  area2 = the sum of x1 y0 - x0 y1 over the loop's edges between their pixel-corner end
points: > 0 for a region's one outer loop, < 0 for a hole loop.

The points of a loop: walk from the leader, take every edge's pixel, merge cyclically consecutive equal pixels, then drop
every point whose step in equals its step out.  A loop around one pixel yields that pixel.

trace(region, sizes, min_pixels, image_base) -> (loops int64 [L, 6], points int32 [P, 2]): loops = {image_base + image,
region root index, leader edge id, n_points, first point, area2} in ascending (image, leader edge id), points = (x, y),
each loop's contiguous and in walk order from its leader.
"""
import numpy as np

DX = (1, 0, -1, 0)
DY = (0, 1, 0, -1)
# the pixel-corner end points of edge d of the pixel at (0, 0): (x0, y0, x1, y1)
CORNERS = ((0, 1, 1, 1), (0, 0, 0, 1), (1, 0, 0, 0), (1, 1, 1, 0))


def _trace_image(reg, keep):
    """[(leader id, root, area2, [(x, y), ...])] of one image, by ascending leader id"""
    h, w = reg.shape

    def member(x, y, v):
        return 0 <= x < w and 0 <= y < h and reg[y, x] == v

    def is_edge(x, y, d):
        r = (d + 1) % 4
        return keep[y, x] and not member(x + DX[r], y + DY[r], reg[y, x])

    def successor(x, y, d):
        v, r = reg[y, x], (d + 1) % 4
        if member(x + DX[d] + DX[r], y + DY[d] + DY[r], v):
            return x + DX[d] + DX[r], y + DY[d] + DY[r], r
        if member(x + DX[d], y + DY[d], v):
            return x + DX[d], y + DY[d], d
        return x, y, (d + 3) % 4

    seen = np.zeros((h, w, 4), bool)
    out = []
    for y in range(h):
        for x in range(w):
            for d in range(4):
                if seen[y, x, d] or not is_edge(x, y, d):
                    continue
                # ascending scan: the first edge of a loop that is met is its leader
                walk, area2, e = [], 0, (x, y, d)
                while not seen[e[1], e[0], e[2]]:
                    seen[e[1], e[0], e[2]] = True
                    assert is_edge(*e)
                    walk.append((e[0], e[1]))
                    c = CORNERS[e[2]]
                    x0, y0, x1, y1 = e[0] + c[0], e[1] + c[1], e[0] + c[2], e[1] + c[3]
                    area2 += x1 * y0 - x0 * y1
                    e = successor(*e)
                assert e == (x, y, d)
                pts = [p for k, p in enumerate(walk) if k == 0 or p != walk[k - 1]]
                while len(pts) > 1 and pts[-1] == pts[0]:
                    pts.pop()
                if len(pts) > 1:
                    m = len(pts)
                    step = [(pts[k][0] - pts[k - 1][0], pts[k][1] - pts[k - 1][1]) for k in range(m)]     # the step in
                    assert all(max(abs(a), abs(b)) == 1 for a, b in step)
                    pts = [pts[k] for k in range(m) if step[k] != step[(k + 1) % m]]
                    assert len(pts) >= 2
                out.append((4 * (y * w + x) + d, int(reg[y, x]) - 1, area2, pts))
    return out


def trace(region, sizes, min_pixels=1, image_base=0):
    region, sizes = np.asarray(region), np.asarray(sizes)
    assert region.ndim == 3 and region.shape == sizes.shape and min_pixels >= 1
    loops, points = [], []
    for i in range(region.shape[0]):
        keep = (region[i] > 0) & (sizes[i] >= min_pixels)
        for leader, root, area2, pts in _trace_image(region[i], keep):
            loops.append((image_base + i, root, leader, len(pts), len(points), area2))
            points.extend(pts)
    return np.array(loops, np.int64).reshape(-1, 6), np.array(points, np.int32).reshape(-1, 2)
