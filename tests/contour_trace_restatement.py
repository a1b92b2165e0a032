"""TEST ONLY: what pp_contour_trace_u8 computes (T1-T7 of platipy_amd/dicom), restated sequentially in plain Python: every
loop is walked crack by crack from its first crack in key order.  Nothing of the kernel's scheme is used -- no ids, no
pointer doubling, no ranking -- and a loop is an outer border or a hole by the SIGN OF ITS ENCLOSED AREA (shoelace over the
cracks' corners), where the kernel reads the leader's side (T3)."""
import numpy as np

N, E, S, W = 0, 1, 2, 3
HEADING = {N: (1, 0), E: (0, 1), S: (-1, 0), W: (0, -1)}      # (dx, dy), y down (T1)
TAIL = {N: (0, 0), E: (1, 0), S: (1, 1), W: (0, 1)}          # the corner a crack starts at, relative to its pixel's corner
ACROSS = {N: (0, -1), E: (1, 0), S: (0, 1), W: (-1, 0)}


def trace_slice(m, approximate=False):
    """m: [ny, nx], foreground where non-zero -> [(leader key (y, x, side), hole, [(x, y), ...]), ...] ordered by leader key."""
    ny, nx = m.shape

    def fg(x, y):
        return 0 <= x < nx and 0 <= y < ny and m[y, x] != 0

    def is_crack(x, y, side):
        ax, ay = ACROSS[side]
        return fg(x, y) and not fg(x + ax, y + ay)

    def successor(x, y, side):      # T2
        dx, dy = HEADING[side]
        arx, ary = x + dx, y + dy
        alx, aly = arx + dy, ary - dx      # left of the heading (dx, dy) as displayed is (dy, -dx)
        if fg(alx, aly):
            return alx, aly, (side + 3) % 4
        if fg(arx, ary):
            return arx, ary, side
        return x, y, (side + 1) % 4

    seen = set()
    out = []
    for y in range(ny):
        for x in range(nx):
            for side in (N, E, S, W):
                if not is_crack(x, y, side) or (y, x, side) in seen:
                    continue
                loop = []      # from the leader: in key order the first crack of a loop we meet is its smallest (T3)
                c = (x, y, side)
                while (c[1], c[0], c[2]) not in seen:
                    assert is_crack(*c)
                    seen.add((c[1], c[0], c[2]))
                    loop.append(c)
                    c = successor(*c)
                assert c == (x, y, side), "a walk must close at its start"
                assert min((cy, cx, cs) for cx, cy, cs in loop) == (y, x, side)
                corners = [(cx + TAIL[cs][0], cy + TAIL[cs][1]) for cx, cy, cs in loop]
                area2 = sum(ax * by - bx * ay for (ax, ay), (bx, by) in zip(corners, corners[1:] + corners[:1]))
                assert area2 != 0
                hole = area2 < 0      # clockwise as displayed (y down) encloses a positive area
                pix = [(cx + ACROSS[cs][0], cy + ACROSS[cs][1]) if hole else (cx, cy) for cx, cy, cs in loop]      # T4
                n = len(pix)
                if all(p == pix[0] for p in pix):      # T5
                    verts = [pix[0]]
                else:
                    k = 0
                    while pix[(k - 1) % n] == pix[k % n]:
                        k -= 1
                    verts = []
                    for j in range(n):
                        p = pix[(k + j) % n]
                        if not verts or p != verts[-1]:
                            verts.append(p)
                if approximate and len(verts) > 2:      # T7
                    v = verts
                    nv = len(v)
                    keep = [(v[i][0] - v[i - 1][0], v[i][1] - v[i - 1][1]) != (v[(i + 1) % nv][0] - v[i][0], v[(i + 1) % nv][1] - v[i][1])
                            for i in range(nv)]
                    verts = [v[i] for i in range(nv) if keep[i]]
                out.append(((y, x, side), hole, verts))
    return out


def trace(masks, approximate=False):
    """masks uint8 [S][Z][Y][X] -> (vertices int32 [n, 2], rows [(first, count, structure, z), ...], hole flags uint8), T6."""
    verts, rows, holes = [], [], []
    for s in range(masks.shape[0]):
        for z in range(masks.shape[1]):
            for _, hole, v in trace_slice(masks[s, z], approximate):
                rows.append((len(verts), len(v), s, z))
                holes.append(int(hole))
                verts += v
    return np.array(verts, dtype=np.int32).reshape(-1, 2), rows, np.array(holes, dtype=np.uint8)
