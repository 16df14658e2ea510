"""The sphere over a floor that tests/test_shadow_ref_cpu.py and tests/test_shadow_gpu.py share: meshes, the light and
the sizes of the geometry test.  numpy only; nothing here touches a device.

The sizes.  The geometry test leaves a band of (r+1) sqrt(2) map texels + 1 voxel about the shadow's rim unchecked and
caps the band at 25 % of the pixels with d < R + band.  With t = R / band the band of a whole disc holds 4 t / (t+1)^2 of
it, 39 % at the largest sphere a 64^2 map holds (R = 31 texels: band = 3.9, t = 8).  So the light's box is fitted to the
sphere alone (the receiver need not lie inside the map: a tap outside it is not occluded), the sphere has radius 0.9,
and the floor is a plank under the shadow's long axis, where the band holds about 2 / (t+1) = 22 % of the pixels."""
import math

import numpy as np

F = np.float32
RES = 65            # the sphere's volume
RADIUS = 0.9        # of the sphere, about the origin
VOXEL = 2.0 / RES
MAP = 64            # the shadow map
FLOOR_Y = -1.0
TILT = math.radians(30.0)
DIRECTION = (math.sin(TILT), -math.cos(TILT), 0.0)  # the light travels down and towards +x
PLANK = ((-1.0, 2.2), (-0.15, 0.15))  # the floor's extent in x and z
BOX = (RADIUS + VOXEL) / math.sqrt(3.0)  # half the side of the light's box: its bounding sphere is the sphere + 1 voxel


def sphere_mesh():
    """(verts [V,3] f32, faces [F,3] int32): the CPU oracle's marching cubes of synthetic.sphere_volume(RES, RADIUS)."""
    from monoport_amd import synthetic
    from oracle import pifu_oracle
    v, f = pifu_oracle.marching_cubes(synthetic.sphere_volume(RES, RADIUS))
    return np.ascontiguousarray(v, F), np.ascontiguousarray(f, np.int32)


def plank(x=PLANK[0], z=PLANK[1], y=FLOOR_Y):
    """A horizontal floor of two triangles: (verts [4,3] f32, faces [2,3] int32, uv [4,2] f32)."""
    verts = np.array([[x[0], y, z[0]], [x[1], y, z[0]], [x[1], y, z[1]], [x[0], y, z[1]]], F)
    uv = np.array([[0, 0], [4, 0], [4, 1], [0, 1]], F)
    return verts, np.array([[0, 1, 2], [0, 2, 3]], np.int32), uv


def light(recon, **kw):
    """``Light.directional`` about the sphere, tilted 30 degrees from the vertical."""
    kw.setdefault("res", MAP)
    return recon.Light.directional(DIRECTION, (-BOX,) * 3, (BOX,) * 3, **kw)


def camera_down(x=PLANK[0], z=PLANK[1]):
    """An orthogonal camera looking down on the plank: the image's first axis is world x, its second world z, its
    depth the height y (nearest = "max": the viewer is above).  [3,4] f32."""
    cx, hx = (x[0] + x[1]) / 2, (x[1] - x[0]) / 2
    cz, hz = (z[0] + z[1]) / 2, (z[1] - z[0]) / 2
    return np.array([[1 / hx, 0, 0, -cx / hx], [0, 0, 1 / hz, -cz / hz], [0, 1, 0, 0]], F)
