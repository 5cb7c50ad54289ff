"""CPU: the region reference against scipy.ndimage.label; link_tracks on hand-written tables; what check_args refuses;
ops.label_regions refuses CPU tensors; the C entry points validate before they launch."""
import numpy as np
import pytest
import torch

import regions_ref as ref

GRIDS = [(1, 1), (1, 7), (2, 2), (5, 7), (2, 130), (33, 65), (1, 1, 1), (1, 1, 9), (2, 2, 2), (5, 6, 7), (9, 9, 33)]


def patterns(sp, seed=0):
    pats = {"empty": np.zeros(sp, bool), "full": np.ones(sp, bool), "checker": ref.checkerboard(sp),
            "serpentine": ref.serpentine(sp), "comb": ref.comb(sp), "diagonal": ref.diagonal(sp), "rings": ref.rings(sp)}
    for p in (0.3, 0.5, 0.6, 0.8):
        pats["random%.1f" % p] = ref.random_fill(sp, p, seed + int(p * 10))
    return pats


@pytest.mark.parametrize("sp", GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_reference_labels_equal_scipy(sp):
    ndi = pytest.importorskip("scipy.ndimage")
    nd = len(sp)
    for name, m in patterns(sp, seed=sum(sp)).items():
        for full in (False, True):
            st = ndi.generate_binary_structure(nd, nd if full else 1)
            want, n = ndi.label(m, structure=st)
            got = ref.label_one(m, full)
            assert np.array_equal(got, ref.canonical(want)), (name, full)
            assert int((got == np.arange(1, m.size + 1).reshape(sp)).sum()) == n, (name, full)


def test_reference_patterns_are_what_they_claim():
    for sp in ((7, 9), (70, 130), (5, 6, 7), (17, 17, 65)):
        nd = len(sp)
        n = lambda m, full: len(np.unique(ref.label_one(m, full))) - 1
        assert n(ref.serpentine(sp), False) == 1 and n(ref.serpentine(sp), True) == 1
        assert ref.serpentine(sp).sum() < 0.75 * np.prod(sp)  # a path, not a slab
        c = ref.checkerboard(sp)
        assert n(c, False) == c.sum() and n(c, True) == 1
        assert n(ref.diagonal(sp), False) == min(sp) and n(ref.diagonal(sp), True) == 1
        assert n(ref.rings(sp), True) == n(ref.rings(sp), False) == (min(sp) - 1) // 6 + 1
        assert n(ref.comb(sp), False) == 1


def test_reference_table_follow_links_by_hand():
    lab = np.zeros((2, 3, 4), np.int32)
    lab[0, 0, :2] = 1
    lab[0, 2, 1:] = 10
    lab[1, 1, :] = 5
    w = np.arange(24, dtype=np.float32).reshape(2, 1, 3, 4) - 3
    t = ref.region_table(lab, w)
    assert t["offsets"].tolist() == [0, 2, 3] and t["label"].tolist() == [1, 10, 5] and t["count"].tolist() == [2, 3, 4]
    assert t["coord_sum"].tolist() == [[0, 1], [6, 6], [4, 6]]
    assert t["bbox"].tolist() == [[[0, 0], [0, 1]], [[2, 1], [2, 3]], [[1, 0], [1, 3]]]
    assert t["wsum"][:, 0].tolist() == [-5.0, 21.0, 58.0] and t["wmin"][:, 0].tolist() == [-3.0, 6.0, 13.0]
    flows = np.zeros((1, 2, 3, 4), np.float32)
    flows[0, 1] = 1.0           # down one row: region 1 lands on 5, region 10 leaves
    flows[0, 0, 0, 1] = 0.5     # x = 1.5 -> 2 (half to even), still on row 1
    flows[0, 0, 0, 0] = np.nan
    d = ref.follow(lab, flows)
    assert d[0, 0].tolist() == [-1, 5, 0, 0] and d[0, 2].tolist() == [0, -1, -1, -1] and (d[0, 1] == 0).all()
    lk = ref.links(lab, d)[0]
    assert lk["src"].tolist() == [0] and lk["dst"].tolist() == [0] and lk["count"].tolist() == [1]
    assert lk["n_out"].tolist() == [1, 3] and lk["n_to_background"].tolist() == [0, 0]
    flows[0, 0] = -0.5          # x - 0.5: 0 -> -0.5 -> -0 (inside), 1 -> 0.5 -> 0, 3 -> 2.5 -> 2
    flows[0, 1] = 0.0
    lab2 = np.stack([lab[1], lab[1]])
    assert ref.follow(lab2, flows)[0, 1].tolist() == [5, 5, 5, 5]


def _table(*sizes):
    off = np.concatenate([[0], np.cumsum([len(s) for s in sizes])])
    return {"count": np.concatenate([np.asarray(s, np.int64) for s in sizes]), "offsets": off}


def _links(n_src, rows, n_out=None, n_bg=None):
    rows = sorted(rows)
    return {"src": np.array([r[0] for r in rows], np.int64), "dst": np.array([r[1] for r in rows], np.int64),
            "count": np.array([r[2] for r in rows], np.int64),
            "n_out": np.array(n_out if n_out is not None else [0] * n_src, np.int64),
            "n_to_background": np.array(n_bg if n_bg is not None else [0] * n_src, np.int64)}


def _events(g):
    return [(e["step"], e["region"], e["event"]) for e in g["events"]]


def test_link_tracks_continuation_split_merge_birth_death():
    from opticalflowscivis_amd.regions import link_tracks
    # step 0: A(10) B(10); step 1: A'(10), B1(5) B2(5), N(4, new); step 2: M(20) = A' + B1 merged; B2 and N die
    tab = _table([10, 10], [10, 5, 5, 4], [20])
    l0 = _links(2, [(0, 0, 10), (1, 1, 5), (1, 2, 5)])
    l1 = _links(4, [(0, 0, 10), (1, 0, 5)], n_bg=[0, 0, 5, 4])
    g = link_tracks(tab, [l0, l1])
    assert g["track_of"][0].tolist() == [1, 2] and g["track_of"][1].tolist() == [1, 2, 3, 4]  # tie 5 == 5: the lower id continues
    assert g["track_of"][2].tolist() == [1]
    assert _events(g) == [(0, 1, "split"), (1, 2, "death"), (1, 3, "birth"), (1, 3, "death"), (2, 0, "merge")]
    t = {t["id"]: t for t in g["tracks"]}
    assert t[1]["regions"] == [(0, 0), (1, 0), (2, 0)] and (t[1]["first"], t[1]["last"]) == (0, 2)
    assert t[2]["regions"] == [(0, 1), (1, 1)] and t[3]["regions"] == [(1, 2)] and t[4]["regions"] == [(1, 3)]
    assert len(g["tracks"]) == 4


def test_link_tracks_mutual_best_and_ties():
    from opticalflowscivis_amd.regions import link_tracks
    # a0 -> b0 (6), a0 -> b1 (6): tie, b0 (lower id) continues; a1 -> b1 (3): b1's best predecessor is a0, whose best
    # successor is b0 -> b1 starts a new track
    tab = _table([12, 3], [6, 9])
    g = link_tracks(tab, [_links(2, [(0, 0, 6), (0, 1, 6), (1, 1, 3)])])
    assert g["track_of"][0].tolist() == [1, 2] and g["track_of"][1].tolist() == [1, 3]
    assert _events(g) == [(0, 0, "split"), (1, 1, "merge")]
    # predecessors tie: a0 -> b0 (4), a1 -> b0 (4): a0 (lower id) is continued
    g = link_tracks(_table([4, 4], [8]), [_links(2, [(0, 0, 4), (1, 0, 4)])])
    assert g["track_of"][1].tolist() == [1] and _events(g) == [(1, 0, "merge")]


def test_link_tracks_thresholds_at_and_below():
    from opticalflowscivis_amd.regions import link_tracks
    tab = _table([8, 3], [8, 4])
    lk = [_links(2, [(0, 0, 2), (1, 1, 3)])]
    # min_overlap 0.25 * min(8, 8) = 2: a count of 2 is kept; 0.26 -> ceil(2.08) = 3: dropped
    assert link_tracks(tab, lk, 1, 0.25)["track_of"][1].tolist() == [1, 2]
    g = link_tracks(tab, lk, 1, 0.26)
    assert g["track_of"][1].tolist() == [3, 2] and (0, 0, "death") in _events(g) and (1, 0, "birth") in _events(g)
    # min_size 3 keeps the region of 3 nodes, 4 drops it, its link and its events
    assert link_tracks(tab, lk, 3, 0.25)["kept"][0].tolist() == [True, True]
    g = link_tracks(tab, lk, 4, 0.25)
    assert g["kept"][0].tolist() == [True, False] and g["track_of"][0].tolist() == [1, 0]
    assert g["track_of"][1].tolist() == [1, 2] and _events(g) == [(1, 1, "birth")]
    assert g["links"][0] == {"src": [0], "dst": [0], "count": [2]}
    # min_overlap 0: any link of at least one node is kept
    assert link_tracks(_table([100], [100]), [_links(1, [(0, 0, 1)])], 1, 0.0)["track_of"][1].tolist() == [1]


def test_link_tracks_exit():
    from opticalflowscivis_amd.regions import link_tracks
    # 10 nodes: 6 leave, 4 land on the next map's region (kept: 4 >= ceil(0.25 * 4)) -> exit, no death; then all leave
    tab = _table([10], [4], [])
    l0 = _links(1, [(0, 0, 4)], n_out=[6])
    l1 = _links(1, [], n_out=[4])
    g = link_tracks(tab, [l0, l1])
    assert _events(g) == [(0, 0, "exit"), (1, 0, "exit"), (1, 0, "death")]
    # most go to background: a death, not an exit
    g = link_tracks(_table([10], []), [_links(1, [], n_out=[3], n_bg=[7])])
    assert _events(g) == [(0, 0, "death")]
    with pytest.raises(ValueError):
        link_tracks(tab, [l0])
    with pytest.raises(ValueError):
        link_tracks(tab, [l0, l1], min_size=0)


def test_check_args_refusals():
    from opticalflowscivis_amd import regions as drv
    ok = lambda argv: drv.check_args(drv._args(2, "x", "rife").parse_args(argv))
    a = ok(["--flows", "f.npy"])
    assert a.weights == "q,vmag" and a.criterion == "q" and a.connectivity == "face" and a.min_size == 1 and a.min_overlap == 0.25
    a = ok(["--flows", "f.npy", "--mask", "m.npy"])
    assert (a.require, a.reject, a.weights) == (1, 128, "")
    for argv in ([], ["--dataset", "droplet2d", "--seq", "s.npy"], ["--flows", "f.npy", "--chunk", "0"],
                 ["--flows", "f.npy", "--min-size", "0"], ["--flows", "f.npy", "--min-overlap", "1.5"],
                 ["--flows", "f.npy", "--min-overlap", "-0.1"], ["--flows", "f.npy", "--dt", "0"],
                 ["--flows", "f.npy", "--spacing", "1", "2", "3"], ["--flows", "f.npy", "--weights", "vort"],
                 ["--flows", "f.npy", "--weights", "q,q"], ["--flows", "f.npy", "--require", "1"],
                 ["--dataset", "droplet2d", "--mask", "m.npy"], ["--flows", "f.npy", "--mask", "m.npy", "--weights", "q"],
                 ["--flows", "f.npy", "--mask", "m.npy", "--require", "256"],
                 ["--flows", "f.npy", "--mask", "m.npy", "--require", "3", "--reject", "1"], ["--flows", "f.npy", "--start", "-1"]):
        with pytest.raises(SystemExit):
            ok(argv)
    with pytest.raises(SystemExit):  # the parser's own
        ok(["--flows", "f.npy", "--criterion", "mask"])
    with pytest.raises(SystemExit):
        ok(["--flows", "f.npy", "--connectivity", "edge"])


def test_ops_refuse_cpu_tensors_and_bad_operands():
    from opticalflowscivis_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.label_regions(torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.region_table(torch.zeros(1, 4, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.region_follow(torch.zeros(2, 4, 4, dtype=torch.int32), torch.zeros(1, 2, 4, 4))
    with pytest.raises(ValueError):
        ops.label_regions(np.zeros((1, 4, 4), np.uint8))
    assert set(ops.REGION_TILE) == {2, 3} and len(ops.REGION_TILE[2]) == 2 and len(ops.REGION_TILE[3]) == 3
    assert ops.regions_cost((8, 16), 3, "label") == (3 * 128 * 5, 0)
    assert ops.regions_cost((8, 16), 3, "stats", F=2) == (3 * 128 * 12, 0)
    assert ops.regions_cost((4, 8, 16), 3, "follow", fg_fraction=0.5) == (2 * (512 * 20 + 4 * 256), 0)
    with pytest.raises(ValueError):
        ops.regions_cost((8, 16), 1, "other")


def test_entry_points_validate_before_launching():
    """NULL -> 1, a zero extent -> 2, an unknown option -> 3: nothing is launched, so no GPU is needed."""
    from opticalflowscivis_amd import _lib
    L = _lib.lib()
    assert L.fs_label_regions2d(None, 1, 8, 8, 64, 1, 128, 0, 1, 1, 1, 1, None) == 1
    assert L.fs_label_regions3d(1, 1, 8, 8, 8, 512, 1, 128, 0, 1, 1, 1, None, None) == 1          # ws NULL
    assert L.fs_label_regions2d(1, 1, 0, 8, 64, 1, 128, 0, 1, 1, 1, 1, None) == 2
    assert L.fs_label_regions3d(1, 1, 8, 0, 8, 512, 1, 128, 0, 1, 1, 1, 1, None) == 2
    assert L.fs_label_regions2d(1, 1, 8, 8, 63, 1, 128, 0, 1, 1, 1, 1, None) == 2                  # stride below a map
    assert L.fs_label_regions3d(1, 1, 2048, 1024, 1024, 1 << 31, 1, 128, 0, 1, 1, 1, 1, None) == 2  # 2^31 nodes
    assert L.fs_label_regions2d(1, 1, 8, 8, 64, 1, 128, 2, 1, 1, 1, 1, None) == 3                  # conn = 2
    assert L.fs_label_regions3d(1, 1, 8, 8, 8, 512, 1, 128, -1, 1, 1, 1, 1, None) == 3
    assert L.fs_label_regions2d(1, 0, 8, 8, 64, 1, 128, 0, 1, 1, 1, 1, None) == 3                  # K < 1
    assert L.fs_label_regions2d(1, 1, 8, 8, 64, 256, 128, 0, 1, 1, 1, 1, None) == 3
    assert L.fs_label_regions2d_ws_bytes(3, 5, 7) == 3 * 35 * 4 and L.fs_label_regions3d_ws_bytes(2, 3, 5, 7) == 2 * 105 * 4
    assert L.fs_label_regions2d_ws_bytes(1, 0, 7) == -2 and L.fs_label_regions3d_ws_bytes(0, 3, 5, 7) == -3
    assert L.fs_region_stats2d(None, 1, 1, None, 1, 0, 8, 8, 1, 1, 1, 1, None, None, None, None) == 1
    assert L.fs_region_stats2d(1, 1, 1, None, 1, 1, 8, 8, 1, 1, 1, 1, 1, 1, 1, None) == 1          # F > 0 without weights
    assert L.fs_region_stats3d(1, 1, 1, None, 1, 0, 8, 8, 0, 1, 1, 1, 1, None, None, None, None) == 2
    assert L.fs_region_stats2d(1, 1, 1, 1, 1, 9, 8, 8, 1, 1, 1, 1, 1, 1, 1, None) == 3             # F > 8
    assert L.fs_region_stats2d(1, 1, 1, None, 1, 0, 8, 8, 0, None, None, None, None, None, None, None) == 0  # R = 0: nothing to do
    assert L.fs_region_follow2d(None, 1, 2, 2, 8, 8, 128, 1, None) == 1
    assert L.fs_region_follow3d(1, 1, 2, 3, 8, 8, 0, 1536, 1, None) == 2
    assert L.fs_region_follow2d(1, 1, 2, 3, 8, 8, 192, 1, None) == 2                               # C != 2
    assert L.fs_region_follow2d(1, 1, 2, 2, 8, 8, 127, 1, None) == 2                               # stride below a field
    assert L.fs_region_follow2d(1, 1, 1, 2, 8, 8, 128, 1, None) == 3                               # K < 2
    big = (1 << 24) + 4  # extent - 1 = 2^24 + 3 is no float: the range test would not be exact
    assert L.fs_region_follow2d(1, 1, 2, 2, 2, big, 4 * big, 1, None) == 2
    assert L.fs_region_follow3d(1, 1, 2, 3, big, 2, 2, 12 * big, 1, None) == 2


def test_link_tracks_many_regions():
    """A map of many small regions (random fill gives 10^5 .. 10^6): the work per region must not grow with their number."""
    from opticalflowscivis_amd.regions import link_tracks
    n = 60000
    ids = np.arange(n, dtype=np.int64)
    tab = {"count": np.full(2 * n, 2, np.int64), "offsets": np.array([0, n, 2 * n])}
    lk = {"src": ids, "dst": ids, "count": np.full(n, 2, np.int64), "n_out": np.zeros(n, np.int64),
          "n_to_background": np.zeros(n, np.int64)}
    lk["n_out"][5] = 1                      # fewer leave than land on the next region: no exit
    lk["n_out"][7], lk["count"][7] = 2, 1   # more nodes leave than land on any one region
    g = link_tracks(tab, [lk])
    assert len(g["tracks"]) == n and _events(g) == [(0, 7, "exit")]
