"""--mst restated in plain Python, from the rule's text (include/bronko_hip.h, bk_cohort_mst) over the matrices of
cohort_ref.distances: Kruskal for the forest, a plain Boruvka for the round count, the rooting and the file's text.

  admissible  a pair {i, j}, i < j, is admissible iff compared[i][j] >= 1 and compared[i][j] >= min_compared
  edge order  (diff, i, j), lexicographically: a strict total order
  forest      what Kruskal keeps: the admissible edges in ascending order, skipping an edge whose ends are already connected
  nearest     nearest[i] = the admissible j != i with the least (diff[i][j], j), or none
  rounds      the Boruvka rounds in which at least one edge was added: every component picks its least outgoing admissible edge
  rooting     a component's root is its smallest sample, every other sample's parent is its neighbour on the path to the root;
              components are numbered from 1 in the order of their first sample
  file        ##mst_min_breadth=B (%g), ##mst_min_compared=C, "sample parent diff compared component size nearest nearest_diff
              nearest_compared", a line per sample; "." for a root's parent, diff and compared and for a missing nearest neighbour
"""
import math

NONE = 0xffffffff


def min_compared(min_breadth, positions):
    """The smallest integer c with float(c) >= min_breadth * float(positions)."""
    return max(0, math.ceil(min_breadth * float(positions)))


def _lists(*matrices):
    return [m.tolist() if hasattr(m, "tolist") else m for m in matrices]


def admissible(compared, i, j, need):
    return i != j and int(compared[i][j]) >= 1 and int(compared[i][j]) >= need


def kruskal(diff, compared, need):
    """The forest's edges [(lo, hi, diff, compared), ...], ascending in the edge order."""
    diff, compared = _lists(diff, compared)
    n = len(diff)
    cand = sorted((int(diff[i][j]), i, j) for i in range(n) for j in range(i + 1, n) if admissible(compared, i, j, need))
    comp = list(range(n))                                        # a sample's component, relabelled in full at every join
    edges = []
    for d, i, j in cand:
        if comp[i] == comp[j]:
            continue
        old, new = comp[j], comp[i]
        comp = [new if c == old else c for c in comp]
        edges.append((i, j, d, int(compared[i][j])))
    return edges


def nearest(diff, compared, need):
    """Per sample (j, diff, compared) of its nearest admissible neighbour, or (NONE, 0, 0)."""
    diff, compared = _lists(diff, compared)
    n = len(diff)
    out = []
    for i in range(n):
        cand = [(int(diff[i][j]), j) for j in range(n) if admissible(compared, i, j, need)]
        if cand:
            d, j = min(cand)
            out.append((j, d, int(compared[i][j])))
        else:
            out.append((NONE, 0, 0))
    return out


def boruvka(diff, compared, need):
    """(edges ascending in the edge order, rounds): every component picks its least outgoing admissible edge, all picked edges are
    merged, until no component has one."""
    diff, compared = _lists(diff, compared)
    n = len(diff)
    comp = list(range(n))
    edges = set()
    rounds = 0
    while True:
        best = {}
        for i in range(n):
            for j in range(n):
                if comp[i] != comp[j] and admissible(compared, i, j, need):
                    key = (int(diff[i][j]), min(i, j), max(i, j))
                    if comp[i] not in best or key < best[comp[i]]:
                        best[comp[i]] = key
        picked = set(best.values()) - edges
        if not picked:
            break
        rounds += 1
        for d, lo, hi in sorted(picked):
            if comp[lo] != comp[hi]:
                old, new = comp[hi], comp[lo]
                comp = [new if c == old else c for c in comp]
            edges.add((d, lo, hi))
    return [(lo, hi, d, int(compared[lo][hi])) for d, lo, hi in sorted(edges)], rounds


def root(n, edges):
    """(parent, diff, compared, component, size) per sample; a root's parent is NONE and its diff and compared are 0."""
    nb = [[] for _ in range(n)]
    for lo, hi, d, c in edges:
        nb[lo].append((hi, d, c))
        nb[hi].append((lo, d, c))
    parent, pd, pc, component, size = [NONE] * n, [0] * n, [0] * n, [0] * n, [0] * n
    number = 0
    for first in range(n):
        if component[first]:
            continue
        number += 1
        component[first] = number
        members, todo = [first], [first]
        while todo:
            i = todo.pop()
            for j, d, c in nb[i]:
                if not component[j]:
                    component[j] = number
                    parent[j], pd[j], pc[j] = i, d, c
                    members.append(j)
                    todo.append(j)
        for i in members:
            size[i] = len(members)
    return parent, pd, pc, component, size


def components_of(n, edges):
    """The samples' component numbers under `edges`: numbered from 1 in the order of their first sample."""
    return root(n, edges)[3]


def mst_text(names, edges, near, min_breadth, need):
    n = len(names)
    parent, pd, pc, component, size = root(n, edges)
    out = ["##mst_min_breadth=%g" % min_breadth, "##mst_min_compared=%d" % need,
           "sample\tparent\tdiff\tcompared\tcomponent\tsize\tnearest\tnearest_diff\tnearest_compared"]
    for i in range(n):
        up = [".", ".", "."] if parent[i] == NONE else [names[parent[i]], str(pd[i]), str(pc[i])]
        nr = [".", ".", "."] if near[i][0] == NONE else [names[near[i][0]], str(near[i][1]), str(near[i][2])]
        out.append("\t".join([names[i]] + up + [str(component[i]), str(size[i])] + nr))
    return ("\n".join(out) + "\n").encode()
