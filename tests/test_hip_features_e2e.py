"""From images to poses and to a cloud with nothing of OpenCV: SfMPipeline.reconstruct_images on six rendered views
against the true poses, and DenseReconstructor.reconstruct(extractor="device") on two views against
reconstruct_from_features on the features FeatureExtractor returns with the dense mode's values."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 320 x 240 at a focal length of 256 pixels from 1 unit away: a pixel covers 0.004 units of the surface, the finer noise
# cell of synthetic._texture (0.0125) three pixels: the texture is not aliased.  8 degrees of arc between views, a relief
# of 0.2 units and a field of view of 64 degrees keep rotation and translation apart.
N_VIEWS, H, W, FOCAL_SCALE, RADIUS, ARC_STEP, RELIEF = 6, 240, 320, 0.8, 1.0, 8.0, 0.2


@pytest.fixture(scope="module")
def scene():
    from amvs import synthetic
    return synthetic.make_scene(N_VIEWS, H, W, seed=7, amp=RELIEF, radius=RADIUS, arc_step_deg=ARC_STEP, focal_scale=FOCAL_SCALE)


def similarity(est, true, centres_est, centres_true):
    """(s, R, t) of the similarity true ~ s R est + t between two sets of poses.  The centres of an arc are nearly
    collinear and leave the rotation about their line open, so R is the rotation nearest to the mean of
    R_true_i^T R_est_i (a view's rotation maps its world to the camera: x_true = R_true^T R_est x_est); s and t then
    follow from the centres by least squares."""
    U, _, Vt = np.linalg.svd(sum(np.asarray(t).T @ np.asarray(e) for e, t in zip(est, true)))
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    a = (R @ centres_est.T).T
    a0, b0 = a - a.mean(0), centres_true - centres_true.mean(0)
    s = (a0 * b0).sum() / (a0 * a0).sum()
    return s, R, centres_true.mean(0) - s * a.mean(0)


def test_sfm_from_images(scene):
    """Measured on the MI355X: all six views registered, 3284 points; the rotation errors after the alignment are 0.28,
    0.21, 0.09, 0.17, 0.28 and 0.15 degrees, a median of 0.19 against the bound of 1 (five times the room); the centres
    lie within 0.2 to 1.1 % of the arc's length of the truth."""
    import amvs
    images = [np.ascontiguousarray(c) for c in scene.colors]
    pipe = amvs.SfMPipeline(scene.camera, fast_mode=True)
    points, colors, poses = pipe.reconstruct_images(images)
    assert sorted(poses) == list(range(N_VIEWS)), f"registered {sorted(poses)}"
    got = np.array([np.ravel(-np.asarray(poses[i].R).T @ np.ravel(poses[i].t)) for i in range(N_VIEWS)])
    true = np.array([np.ravel(scene.poses[i].center) for i in range(N_VIEWS)])
    s, R, t = similarity([poses[i].R for i in range(N_VIEWS)], [scene.poses[i].R for i in range(N_VIEWS)], got, true)
    centre = np.linalg.norm((s * (R @ got.T)).T + t - true, axis=1) / np.linalg.norm(true[-1] - true[0])
    rot = []
    for i in range(N_VIEWS):
        rel = np.asarray(poses[i].R) @ R.T @ np.asarray(scene.poses[i].R).T          # the aligned rotation against the truth
        rot.append(np.degrees(np.arccos(np.clip((np.trace(rel) - 1.0) / 2.0, -1.0, 1.0))))
    print(f"SfM from images: {len(points)} points; rotation error median {np.median(rot):.4f} max {np.max(rot):.4f} degrees; "
          f"centre error median {np.median(centre):.5f} max {np.max(centre):.5f} of the arc")
    assert len(points) > 50 and np.median(rot) < 1.0


def test_dense_mode_from_images(scene):
    import amvs
    images = [{"gray": (np.clip(np.rint(scene.grays[i] * 255.0), 0, 255)).astype(np.uint8), "image": scene.colors[i]} for i in range(2)]
    poses = {i: scene.poses[i] for i in range(2)}
    dense = amvs.DenseReconstructor(scene.camera)
    pts, col = dense.reconstruct(images, poses, extractor="device")
    assert len(pts) > 0 and len(col) == len(pts)
    with dense.device_extractor() as ex:
        features = {i: {"points": f.points, "descriptors": f.descriptors} for i, f in ((i, ex.extract(images[i]["gray"])) for i in range(2))}
    assert ex._engine is None
    assert all(len(f["points"]) > 100 for f in features.values())
    pts2, col2 = dense.reconstruct_from_features(features, images, poses)
    assert np.array_equal(pts, pts2) and np.array_equal(col, col2)
