"""Host-built edge tables of the GPU engine (csrc/megba/gpu/edge_tables.hpp)
through the _core.gpu_edge_tables debug binding: the run-aligned window table
of the fused Schur kernels and the point-band camera chunk table.  No GPU is
involved; every expected structure is rebuilt here in numpy.
"""
import numpy as np

from megba_amd import _core


def _edges_from_degrees(deg):
    """Point p is seen by cameras 0..deg[p]-1, edges in shuffled order."""
    pi = np.repeat(np.arange(len(deg)), deg)
    ci = np.concatenate([np.arange(d) for d in deg])
    perm = np.random.default_rng(0).permutation(len(pi))
    return ci[perm].astype(np.int32), pi[perm].astype(np.int32), int(max(deg))


def _tables(ci, pi, ncam, npt, **kw):
    t = _core.gpu_edge_tables(ci, pi, ncam, npt, **kw)
    order = np.lexsort((ci, pi))  # primary order: by point, then camera
    e0, e1 = t["e0"], t["e1"]
    np.testing.assert_array_equal(t["pt_of"], pi[order][e0:e1])
    np.testing.assert_array_equal(t["cam_of"], ci[order][e0:e1])
    return t


def _ref_windows(deg, pt0=0):
    """Greedy reference: (lo, hi, flag) per window and the long points."""
    wins, longs, pos, open_ = [], [], 0, False
    for p, d in enumerate(deg):
        if d > 64:
            longs.append(pt0 + p)
            wins += [(s, min(s + 64, pos + d), 1)
                     for s in range(pos, pos + d, 64)]
            open_ = False
        elif open_ and wins[-1][1] - wins[-1][0] + d <= 64:
            wins[-1] = (wins[-1][0], pos + d, 0)
        else:
            wins.append((pos, pos + d, 0))
            open_ = True
        pos += d
    return wins, longs


def _check_windows(t, deg_local):
    """Structural properties, independent of the merge policy."""
    lo, hi, flag = t["win_lo"], t["win_hi"], t["win_flag"]
    nl = t["e1"] - t["e0"]
    # every local edge lies in exactly one window
    assert lo[0] == 0 and hi[-1] == nl
    np.testing.assert_array_equal(lo[1:], hi[:-1])
    assert (hi > lo).all() and (hi - lo <= 64).all()
    ptr = np.concatenate([[0], np.cumsum(deg_local)])
    pt_lo = t["pt_lo"]
    long_pts = pt_lo + np.flatnonzero(np.asarray(deg_local) > 64)
    np.testing.assert_array_equal(t["long_pts"], long_pts)
    np.testing.assert_array_equal(t["flag_wins"], np.flatnonzero(flag))
    # unflagged windows cover whole runs of short points only
    for a, b in zip(lo[flag == 0], hi[flag == 0]):
        assert a in ptr and b in ptr
        pts = np.flatnonzero((ptr[:-1] >= a) & (ptr[:-1] < b))
        assert (np.asarray(deg_local)[pts] <= 64).all()
    # a long run is cut into consecutive flagged windows of <= 64 edges
    for p in long_pts - pt_lo:
        cuts = list(range(ptr[p], ptr[p + 1], 64))
        idx = np.flatnonzero((lo >= ptr[p]) & (lo < ptr[p + 1]))
        np.testing.assert_array_equal(lo[idx], cuts)
        np.testing.assert_array_equal(hi[idx], cuts[1:] + [ptr[p + 1]])
        assert flag[idx].all()


def _assert_windows_equal(t, deg_local):
    wins, longs = _ref_windows(deg_local, t["pt_lo"])
    np.testing.assert_array_equal(t["win_lo"], [w[0] for w in wins])
    np.testing.assert_array_equal(t["win_hi"], [w[1] for w in wins])
    np.testing.assert_array_equal(t["win_flag"], [w[2] for w in wins])
    np.testing.assert_array_equal(t["long_pts"], longs)
    _check_windows(t, deg_local)


def test_windows_degrees_around_64():
    deg = [1, 63, 64, 65, 128, 129, 3, 2]
    ci, pi, ncam = _edges_from_degrees(deg)
    t = _tables(ci, pi, ncam, len(deg))
    _assert_windows_equal(t, deg)
    # 1 + 63 merge into one full window; 64 stands alone; 65 -> 64 + 1;
    # 128 -> 64 + 64; 129 -> 64 + 64 + 1; 3 + 2 merge
    np.testing.assert_array_equal(
        t["win_hi"] - t["win_lo"], [64, 64, 64, 1, 64, 64, 64, 64, 1, 5])
    np.testing.assert_array_equal(t["long_pts"], [3, 4, 5])


def test_windows_merge_boundary():
    # short runs summing to exactly 64 share a window, 65 does not; the
    # long run in between closes the open window
    deg = [20, 20, 24, 70, 20, 20, 25, 64, 1]
    ci, pi, ncam = _edges_from_degrees(deg)
    t = _tables(ci, pi, ncam, len(deg))
    _assert_windows_equal(t, deg)
    np.testing.assert_array_equal(
        t["win_hi"] - t["win_lo"], [64, 64, 6, 40, 25, 64, 1])
    np.testing.assert_array_equal(t["win_flag"], [0, 1, 1, 0, 0, 0, 0])


def test_windows_two_rank_split():
    deg = [5, 66, 30, 30, 4, 1, 64, 65, 7, 60, 4, 3, 130, 2]
    ci, pi, ncam = _edges_from_degrees(deg)
    covered = 0
    for rank in range(2):
        t = _tables(ci, pi, ncam, len(deg), rank=rank, world=2)
        assert t["e0"] == covered  # ranks tile the edges, point-aligned
        covered = t["e1"]
        assert t["pt_hi"] > t["pt_lo"]
        _assert_windows_equal(t, deg[t["pt_lo"]:t["pt_hi"]])
    assert covered == sum(deg)


def _chunk_problem():
    rng = np.random.default_rng(5)
    ncam, npt = 5, 30
    seen = rng.random((npt, ncam)) < 0.6
    seen[np.arange(npt), rng.integers(0, ncam, npt)] = True
    pi, ci = np.nonzero(seen)
    perm = rng.permutation(len(pi))
    return ci[perm].astype(np.int32), pi[perm].astype(np.int32), ncam, npt


def _ref_chunks(cam_of, pt_of, ncam, chunk_rows, band_pts):
    order = np.argsort(cam_of, kind="stable")  # cam-sorted rows
    pt_of_cam = pt_of[order]
    cam_pos = np.empty_like(order)
    cam_pos[order] = np.arange(len(order))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam_of,
                                                         minlength=ncam))])
    chunks = []
    for c in range(ncam):
        rows = np.arange(row_ptr[c], row_ptr[c + 1])
        band = pt_of_cam[rows] // band_pts
        for b in np.unique(band):
            r = rows[band == b]
            chunks += [(b, c, s, min(s + chunk_rows, r[-1] + 1))
                       for s in range(r[0], r[-1] + 1, chunk_rows)]
    chunks.sort(key=lambda ch: ch[0])  # stable: band-major, cut order kept
    return cam_pos, pt_of_cam, np.array(chunks), row_ptr


def test_chunks_banded():
    ci, pi, ncam, npt = _chunk_problem()
    chunk_rows, band_pts = 4, 10
    t = _tables(ci, pi, ncam, npt, chunk_rows=chunk_rows, band_pts=band_pts)
    cam_of, pt_of = t["cam_of"], t["pt_of"]
    cam_pos, pt_of_cam, ref, row_ptr = _ref_chunks(cam_of, pt_of, ncam,
                                                   chunk_rows, band_pts)
    nl = len(cam_of)
    # camPos is a permutation onto the cam-sorted rows
    np.testing.assert_array_equal(np.sort(t["cam_pos"]), np.arange(nl))
    np.testing.assert_array_equal(t["pt_of_cam"][t["cam_pos"]], pt_of)
    np.testing.assert_array_equal(t["cam_pos"], cam_pos)
    np.testing.assert_array_equal(t["pt_of_cam"], pt_of_cam)
    ch_cam, lo, hi = t["ch_cam"], t["ch_lo"], t["ch_hi"]
    # [chLo, chHi) tile every camera's rows exactly once
    hits = np.zeros(nl, int)
    for c, a, b in zip(ch_cam, lo, hi):
        assert row_ptr[c] <= a < b <= row_ptr[c + 1]
        hits[a:b] += 1
    assert (hits == 1).all()
    # no chunk exceeds chunk_rows or crosses a band boundary
    assert (hi - lo <= chunk_rows).all()
    band_lo = pt_of_cam[lo] // band_pts
    band_hi = pt_of_cam[hi - 1] // band_pts
    np.testing.assert_array_equal(band_lo, band_hi)
    assert len(np.unique(band_lo)) >= 3
    # some (camera, band) group is actually cut by chunk_rows
    assert len(lo) > len(set(zip(ch_cam.tolist(), band_lo.tolist())))
    # band-major, original (camera, row) order kept within a band
    assert (np.diff(band_lo) >= 0).all()
    for b in np.unique(band_lo):
        assert (np.diff(lo[band_lo == b]) > 0).all()
    np.testing.assert_array_equal(np.stack([band_lo, ch_cam, lo, hi], 1), ref)


def test_chunks_single_band_is_unbanded_cut():
    ci, pi, ncam, npt = _chunk_problem()
    for band_pts in (0, npt, 10 * npt):
        t = _tables(ci, pi, ncam, npt, chunk_rows=4, band_pts=band_pts)
        row_ptr = np.concatenate(
            [[0], np.cumsum(np.bincount(t["cam_of"], minlength=ncam))])
        ref = [(c, s, min(s + 4, row_ptr[c + 1])) for c in range(ncam)
               for s in range(row_ptr[c], row_ptr[c + 1], 4)]
        np.testing.assert_array_equal(
            np.stack([t["ch_cam"], t["ch_lo"], t["ch_hi"]], 1), ref)


def test_chunks_two_rank_split():
    ci, pi, ncam, npt = _chunk_problem()
    for rank in range(2):
        t = _tables(ci, pi, ncam, npt, rank=rank, world=2, chunk_rows=4,
                    band_pts=10)
        cam_pos, pt_of_cam, ref, _ = _ref_chunks(t["cam_of"], t["pt_of"],
                                                 ncam, 4, 10)
        np.testing.assert_array_equal(t["cam_pos"], cam_pos)
        got = np.stack([t["pt_of_cam"][t["ch_lo"]] // 10, t["ch_cam"],
                        t["ch_lo"], t["ch_hi"]], 1)
        np.testing.assert_array_equal(got, ref)
