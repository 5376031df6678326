"""Real CU partitions for the frame pass on a partition: the luma CU tree of a picture
of a committed stream fixture (tests/golden/stream_<name>.npz), as the reference encoder
chose it.

TEST INFRASTRUCTURE."""
import numpy as np

from stream_fixture import StreamFixture


def luma_partition(fix, picture):
    """(n, 4) int32 array of (x, y, w, h): the CUs of `picture`'s luma tree (records with
    tree == 0) in coding order, clipped to the picture.  fix: a StreamFixture or its name."""
    if isinstance(fix, str):
        fix = StreamFixture(fix)
    info = fix.info[picture]
    W, H = int(info["width"]), int(info["height"])
    cus = fix.cus(picture)
    cus = cus[cus["tree"] == 0]
    x, y = cus["x"].astype(np.int32), cus["y"].astype(np.int32)
    w = np.minimum(cus["w"].astype(np.int32), W - x)
    h = np.minimum(cus["h"].astype(np.int32), H - y)
    return np.stack([x, y, w, h], axis=1).astype(np.int32)


def picture_size(fix, picture):
    if isinstance(fix, str):
        fix = StreamFixture(fix)
    info = fix.info[picture]
    return int(info["width"]), int(info["height"])
