"""Camera paths for free-pose rendering: host numpy in float64, no scipy.  A path is a few hundred poses, computed once and uploaded once as
float32 (`DeviceScene.sample_pose` / `UCNeRFSystem.render_path` take it from there); nothing here is a kernel or touches a device.

The reference's spiral and spherical generators (utils/utils.py: gen_render_path and friends) are not mirrored; `interp_path` is the plain
keyframe interpolation its `interp_poses` stands for, written out: quaternion slerp for the rotations, linear translations.
"""
import numpy as np


def quat_from_matrix(R):
    """Unit quaternion (w, x, y, z) of a 3 x 3 rotation matrix, float64: the branch with the largest pivot (Shepperd), normalised.  The sign is
    whatever that branch gives; `slerp` takes the shorter arc, so it does not matter."""
    R = np.asarray(R, dtype=np.float64)
    t = np.trace(R)
    if t > 0.0:
        s = np.sqrt(t + 1.0) * 2.0
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2.0
        q = np.empty(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return q / np.linalg.norm(q)


def matrix_from_quat(q):
    """3 x 3 rotation matrix of a quaternion (w, x, y, z), normalised first: orthonormal to rounding."""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def slerp(q0, q1, t):
    """Spherical interpolation from q0 (t = 0) to q1 (t = 1) along the SHORTER arc: q1 is negated when q0 . q1 < 0 (q and -q are one
    rotation).  Nearly parallel quaternions (sin of the angle below 1e-8) are interpolated linearly.  The result is normalised."""
    q0, q1 = np.asarray(q0, dtype=np.float64), np.asarray(q1, dtype=np.float64)
    d = float(np.dot(q0, q1))
    if d < 0.0:
        q1, d = -q1, -d
    d = min(d, 1.0)
    theta = np.arccos(d)
    s = np.sin(theta)
    if s < 1e-8:
        q = (1.0 - t) * q0 + t * q1
    else:
        q = (np.sin((1.0 - t) * theta) / s) * q0 + (np.sin(t * theta) / s) * q1
    return q / np.linalg.norm(q)


def interp_path(c2ws, n):
    """`n` poses along the keyframes c2ws [K,3,4] (camera-to-world) -> float64 [n,3,4].  The parameter is uniform over the K - 1 segments:
    pose j sits at u_j = j / (n - 1), that is at s = u_j (K - 1), in segment floor(s) at the fraction s - floor(s) (formed from the integers
    j (K - 1) and n - 1, so a pose that falls on a keyframe falls on it exactly).  Rotations: quaternion slerp along the shorter arc;
    translations: linear.  A pose at fraction 0 (or 1) IS the keyframe, copied, its rotation block as given even when that is not orthonormal:
    the first and the last pose are the first and the last keyframe, and with n - 1 a multiple of K - 1 every keyframe is reproduced exactly.
    n = 1 returns the first keyframe alone, [1,3,4]; K = 1 returns n copies of the one keyframe.  n < 1 or K < 1 is a ValueError."""
    c2ws = np.asarray(c2ws, dtype=np.float64)
    n = int(n)
    if c2ws.ndim != 3 or c2ws.shape[1:] != (3, 4) or c2ws.shape[0] < 1:
        raise ValueError("interp_path: keyframes must be [K,3,4] with K >= 1, got %s" % (c2ws.shape,))
    if n < 1:
        raise ValueError("interp_path: n = %d poses, expected at least 1" % n)
    K = c2ws.shape[0]
    if n == 1 or K == 1:
        return np.repeat(c2ws[:1], n, axis=0)
    quats = [quat_from_matrix(c[:, :3]) for c in c2ws]
    out = np.empty((n, 3, 4))
    for j in range(n):
        seg, rem = divmod(j * (K - 1), n - 1)
        if seg == K - 1:
            seg, rem = K - 2, n - 1
        if rem == 0:
            out[j] = c2ws[seg]
        elif rem == n - 1:
            out[j] = c2ws[seg + 1]
        else:
            f = rem / (n - 1)
            out[j, :, :3] = matrix_from_quat(slerp(quats[seg], quats[seg + 1], f))
            out[j, :, 3] = (1.0 - f) * c2ws[seg, :, 3] + f * c2ws[seg + 1, :, 3]
    return out
