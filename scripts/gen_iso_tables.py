"""Derives the triangle table of the marching-tetrahedra kernels (opticalflowscivis_amd/csrc/iso_tables.hpp) from the
definition in include/flowsci_hip.h ("Isosurfaces"): nothing in that file is typed in by hand.

    python scripts/gen_iso_tables.py            # print the header
    python scripts/gen_iso_tables.py --write    # rewrite opticalflowscivis_amd/csrc/iso_tables.hpp

A cell's six tetrahedra are the permutations of the axes (x = 0, y = 1, z = 2) in lexicographic order; tetrahedron pi has
the corners c0 = origin, c1 = c0 + e_pi0, c2 = c1 + e_pi1, c3 = origin + (1,1,1).  A case is the 4-bit number whose bit i
says corner i is inside.  The six edges of a tetrahedron are numbered (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) -> 0..5.  One
table word: bits 0-1 the number of triangles, bits 2-10 the three edge numbers of the first triangle (3 bits each, first
vertex lowest), bits 11-19 those of the second.  tests/test_isosurface_cpu.py checks the committed header against this
script and against the restatement's own geometry."""
import itertools
import os
import sys

PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
PERMS = tuple(itertools.permutations((0, 1, 2)))


def corners(perm):
    """Corners of tetrahedron `perm` in (x, y, z)."""
    c = [[0, 0, 0]]
    for a in perm[:2]:
        n = list(c[-1])
        n[a] += 1
        c.append(n)
    return c + [[1, 1, 1]]


def _sub(a, b):
    return [x - y for x, y in zip(a, b)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def triangles(perm, case):
    """Triangles of tetrahedron `perm` in `case`: lists of three edge numbers, oriented towards the outside corners."""
    ins = [i for i in range(4) if case >> i & 1]
    outs = [i for i in range(4) if not case >> i & 1]
    if not ins or not outs:
        return []
    E = lambda p, q: PAIRS.index((min(p, q), max(p, q)))
    if len(ins) == 2:
        q = [E(ins[0], outs[0]), E(ins[0], outs[1]), E(ins[1], outs[1]), E(ins[1], outs[0])]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    else:
        s = ins[0] if len(ins) == 1 else outs[0]
        tris = [[E(s, o) for o in range(4) if o != s]]
    c = corners(perm)
    # (all coordinates doubled and summed, so that everything stays an integer)
    mid = [[a + b for a, b in zip(c[p], c[q])] for p, q in PAIRS]
    direction = [len(ins) * sum(c[o][r] for o in outs) - len(outs) * sum(c[i][r] for i in ins) for r in range(3)]
    out = []
    for t in tris:
        n = _cross(_sub(mid[t[1]], mid[t[0]]), _sub(mid[t[2]], mid[t[0]]))
        d = sum(a * b for a, b in zip(n, direction))
        assert d != 0
        out.append(t if d > 0 else [t[0], t[2], t[1]])
    return out


def word(perm, case):
    tris = triangles(perm, case)
    w = len(tris)
    for j, t in enumerate(tris):
        for i, e in enumerate(t):
            w |= e << (2 + 9 * j + 3 * i)
    return w


def render():
    lines = ["// iso_tables.hpp -- written by scripts/gen_iso_tables.py from the definition in include/flowsci_hip.h; do not edit.",
             "// kIsoTri[tetrahedron][case]: bits 0-1 triangles, bits 2-10 and 11-19 their three edge numbers (3 bits each);",
             "// a tetrahedron's edges (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) are numbered 0..5, case bit i = corner i inside.",
             "#pragma once",
             "__device__ static const unsigned kIsoTri[6][16] = {"]
    for perm in PERMS:
        lines.append("    {" + ", ".join("0x%05xu" % word(perm, cs) for cs in range(16)) + "},  // pi = %d%d%d" % perm)
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = render()
    if "--write" in sys.argv[1:]:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        with open(os.path.join(root, "opticalflowscivis_amd", "csrc", "iso_tables.hpp"), "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
