"""Files whose blocks are more than one channel or time point deep, read on a
machine with a GPU: the pipelined GPU decode copies a chunk down as a run of
frames, which such blocks do not fill, so these files go to the host reader
(tests/test_library_cpu.py has the same files; without a GPU they always did)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bs", [[16, 16, 3, 2, 1], [16, 8, 2, 1, 2]], ids=["c2", "t2"])
def test_whole_image_and_device_destination(lfmlib, oracle, gpu, tmp_path, bs):
    img = oracle.synthetic_lf(37, 29, Z=5, C=2, Tn=3, T=7)
    p = str(tmp_path / "deep.lfm")
    lfmlib.write_lfm(p, img, predictor_request=8, nnum=7, block_size=bs)
    back, _, _ = lfmlib.read_lfm(p)
    assert np.array_equal(back, img)
    d, st = lfmlib.read_lfm_device(p, return_stats=True)
    assert st["path"] == 1, st
    assert np.array_equal(d.cpu().view(gpu.int16).numpy().view(np.uint16), img)
