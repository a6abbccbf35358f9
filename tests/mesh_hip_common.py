"""What the GPU mesh tests (test_hip_mesh*.py) share word for word (a helper module, not a conftest): the context
they run on, the bit-for-bit comparisons and the inputs of the end-to-end tests on scene_a.  A helper that differs
from file to file (every file's Source, the render tests' engine and comparisons) stays in its file."""
import numpy as np

K_ANY = np.array([[30.0, 0, 16.0], [0, 30.0, 12.0], [0, 0, 1]], np.float32)


def _engine(H=24, W=32, n=1, K=K_ANY):
    import amvs
    return amvs.Engine(H, W, n, K)


def _same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_mesh_equal(mesh, ref, what):
    verts, faces, cols = mesh[:3]
    rv, rf, rc = ref[:3]
    assert (len(verts), len(faces)) == (len(rv), len(rf)), f"{what}: {len(verts)} / {len(faces)} vs {len(rv)} / {len(rf)}"
    assert verts.shape == (len(rv), 3) and faces.shape == (len(rf), 3) and cols.shape == (len(rv), 3)
    assert np.array_equal(faces, rf), f"{what}: faces differ, first at {np.argwhere(faces != rf)[:1]}"
    assert _same_bits(verts, rv), f"{what}: vertex positions differ in {int((verts != rv).any(axis=1).sum())} vertices"
    assert np.array_equal(cols, rc), f"{what}: vertex colours differ"


def _scene_a_inputs(scene_a):
    """Images, poses and sparse points (the ground-truth depth of view 0, every 8th pixel) of the committed scene."""
    import amvs
    images = [{"image": np.ascontiguousarray(c)} for c in scene_a.colors]
    d = scene_a.gt_depth[0][::8, ::8].astype(np.float64)
    ys, xs = np.mgrid[0:scene_a.H:8, 0:scene_a.W:8]
    rays = np.stack([xs, ys, np.ones_like(xs)], -1).reshape(-1, 3) @ np.linalg.inv(scene_a.K).T
    sparse = (rays * d.reshape(-1, 1) - scene_a.t[0]) @ scene_a.R[0]
    return amvs.Camera(K=scene_a.K.copy(), dist=np.zeros(5)), images, scene_a.poses(), sparse
