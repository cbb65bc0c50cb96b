"""Prints the two constant tables of cloudaae_amd/csrc/tsdf.hip ("Fused models"): paste the output over the
block between the `generated` markers of that file.

    python tools/gen_tsdf_tables.py

TSDF_EDGES[16]  per sign pattern of a tetrahedron (bit l: local vertex l is inside) its triangles before the swap: vertex v
                of triangle t is the edge (la, lb), la < lb, in bits 12 t + 4 v .. + 3 as la | lb << 2.
TSDF_SWAP[6]    per tetrahedron a 16-bit mask: bit p set = the second and third vertices of pattern p's triangles are
                swapped, so that the normal (p1 - p0) x (p2 - p0) points from the inside vertices towards the outside ones.

The swap is decided here on the unit cell with every vertex at the middle of its edge, as an exact integer determinant
(coordinates doubled); tests/fuse_reference.py decides it again, by another route, and the GPU tests compare the two through
the kernels' output."""
import itertools


def tetrahedra():
    return [(0, 1 << a1, (1 << a1) | (1 << a2), 7) for a1, a2, _ in itertools.permutations(range(3))]


def triangles(p):
    ins = [l for l in range(4) if (p >> l) & 1]
    outs = [l for l in range(4) if not (p >> l) & 1]
    if not ins or not outs:
        return []
    if len(ins) == 1 or len(outs) == 1:
        s = ins[0] if len(ins) == 1 else outs[0]
        return [[(min(s, o), max(s, o)) for o in range(4) if o != s]]
    (a, b), (c, d) = ins, outs
    q = [(min(e), max(e)) for e in ((a, c), (a, d), (b, d), (b, c))]
    return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]


def xyz(c):
    return (c & 1, (c >> 1) & 1, c >> 2)


def swapped(tet, p):
    ins = [l for l in range(4) if (p >> l) & 1]
    outs = [l for l in range(4) if not (p >> l) & 1]
    # (inside mean - outside mean) times len(ins) * len(outs): integers
    toward = [len(outs) * sum(xyz(tet[l])[a] for l in ins) - len(ins) * sum(xyz(tet[l])[a] for l in outs) for a in range(3)]
    answers = set()
    for tri in triangles(p):
        pts = [[xyz(tet[la])[a] + xyz(tet[lb])[a] for a in range(3)] for la, lb in tri]      # midpoints, doubled
        e1 = [pts[1][a] - pts[0][a] for a in range(3)]
        e2 = [pts[2][a] - pts[0][a] for a in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        dot = sum(n[a] * toward[a] for a in range(3))
        assert dot != 0
        answers.add(dot > 0)
    assert len(answers) == 1
    return answers.pop()


def main():
    edges = []
    for p in range(16):
        word = 0
        for t, tri in enumerate(triangles(p)):
            for v, (la, lb) in enumerate(tri):
                word |= (la | (lb << 2)) << (12 * t + 4 * v)
        edges.append(word)
    swaps = [sum(1 << p for p in range(1, 15) if swapped(tet, p)) for tet in tetrahedra()]
    print("__constant__ unsigned int TSDF_EDGES[16] = {%s};" % ", ".join("0x%06xu" % w for w in edges))
    print("__constant__ unsigned int TSDF_SWAP[6] = {%s};" % ", ".join("0x%04xu" % w for w in swaps))


if __name__ == "__main__":
    main()
