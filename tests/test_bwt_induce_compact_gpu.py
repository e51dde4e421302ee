"""The compact induction scan of the GPU bzip2 encoder (bwt_bucket's live
counts, bwt_place_sorted, bwt_induce) against the reference bzip2, byte for
byte, on the stream shapes of test_bwt_induce_compact_cpu.  Every
non-periodic stream must come back with flags == 0: a stream handed to the
host library would hide a wrong scan."""
import numpy as np
import pytest

import test_bwt_induce_compact_cpu as M

pytestmark = pytest.mark.gpu

SHAPES = M.shapes()


def ref_bz2(oracle, data, level):
    """The reference's own bzip2-1.0.6 (oracle/_ref/libbz2_ref.so)."""
    bz = oracle.bzip2()
    assert "reference" in bz.kind, "oracle/_ref/libbz2_ref.so missing: run make -C oracle"
    return bz.compress(bytes(data), level)


def encode(lfmlib, torch, rows):
    """One batch: equal-length streams, one per row, level 2."""
    rows = [np.asarray(r, np.uint8) for r in rows]
    n = len(rows[0])
    assert all(len(r) == n for r in rows)
    d = torch.from_numpy(np.concatenate(rows)).cuda()
    return lfmlib.bzip2_device(d, [n, 1, len(rows), 1, 1], [n, 1, 1, 1, 1], 1, level=2)


@pytest.mark.parametrize("name,raw,want", SHAPES, ids=[s[0] for s in SHAPES])
def test_stream_shape_matches_reference(lfmlib, oracle, gpu, name, raw, want):
    T = M.rle1(raw)
    mode = M.kernel_mode(T)
    assert not M.is_periodic(T) and (want is None or mode == want)
    print("%s: %d bytes, text %d, mode %d, compact length %d, rotation 0 %s" %
          (name, len(raw), len(T), mode, M.compact_length(T, mode), M.rot0_role(T, mode)))
    got, flags = encode(lfmlib, gpu, [raw])
    assert flags[0] == 0, name
    assert got[0] == ref_bz2(oracle, raw.tobytes(), 2), name


@pytest.mark.parametrize("with_periodic", [False, True])
def test_mixed_batch_of_modes(lfmlib, oracle, gpu, with_periodic):
    """kModeSortA, kModeSortB and kModeFull (a long 0xFB run) streams side by
    side in one batch; then with a periodic stream among them (its equal
    rotations make the encoder sort that whole batch again, every rotation)."""
    n = 6000
    rng = np.random.default_rng(11)
    rows = {
        "sort_a": M.bench_like(n, 12),
        "sort_b": M.triples_b(n, 13),
        "full": np.concatenate([np.full(3000, 0xFB, np.uint8), rng.integers(0, 256, n - 3000).astype(np.uint8)]),
        "periodic": np.tile(np.array([7, 1, 200, 3, 3, 90], np.uint8), n // 6),
        "sort_a_live": M.ascending_runs(n, 14),
    }
    if not with_periodic:
        del rows["periodic"]
    modes = {k: M.kernel_mode(M.rle1(v)) for k, v in rows.items() if k != "periodic"}
    assert modes == {"sort_a": M.SORT_A, "sort_b": M.SORT_B, "full": M.FULL, "sort_a_live": M.SORT_A}
    assert not with_periodic or M.is_periodic(M.rle1(rows["periodic"]))
    names = list(rows)
    got, flags = encode(lfmlib, gpu, [rows[k] for k in names])
    for i, k in enumerate(names):
        if k == "periodic":
            assert flags[i], "a periodic stream goes to the host library"
            continue
        assert flags[i] == 0, k
        assert got[i] == ref_bz2(oracle, rows[k].tobytes(), 2), k
