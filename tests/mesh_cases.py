"""The catalogue of mesh cases shared by tests/test_scene_mesh.py (properties of the restatement) and
tests/test_scene_mesh_gpu.py (the kernels against the restatement): the surface cases of tests/surface_cases.py that bear
on a mesh, and a few of its own.  `expected(name, visible_only)` is the restatement's mesh, computed once; `images(name)`
are the case's seeded images.

Maps of 2 x 2 (one cell), 2 x 3, 3 x 3, 3 x 4, 5 x 4 (less than one wave) and 48 x 48 (2304 points: nine slices of 256;
4418 triangles: seventeen slices and a ragged eighteenth); frames of 5 x 7 to 96 x 128 pixels; one to twelve frames.
"""
import functools

import numpy as np

import mesh_restatement
import surface_cases
from surface_cases import SHAPES, _case, at_pixels, plane


def spike_case():
    """Three frames, boxes in the first one only: an empty frame in the middle and one at the end.  Box 0: a 3 x 3 plane
    whose CENTRE vertex lies 5 m behind it: valid, but each of its six triangles spans more than max_edge_dz = 1 and is
    dropped, so it is no vertex -- and nor are the corners (0, 2) and (2, 0), whose triangles all touch the centre.  Two
    triangles and six vertices remain.  Box 1: a whole 3 x 3 plane in front of its middle."""
    z = np.full((3, 3), 4.0)
    z[1, 1] = 9.0
    rows, cols = np.meshgrid(1 + 2 * np.arange(3), 1 + 2 * np.arange(3), indexing='ij')
    return _case([at_pixels(cols, rows, z), plane(2, 2, 1, 1, 3, 3, z=2.0)],
                 [0, 0], [(7, 7), SHAPES[0], SHAPES[1]])


def hidden_case():
    """Box 0, a small plane at 8 m, lies wholly behind box 1 at 2 m: with visible_only it gives no face and no vertex,
    and the offsets of the boxes behind it go on from where it stands.  Box 2 is alone in the second frame; the third
    frame has no box."""
    far = plane(3, 3, 1, 1, 3, 3, z=8.0)
    near = plane(1, 1, 3, 3, 3, 3, z=2.0)
    return _case([far, near, plane(0, 0, 2, 2, 3, 3)], [0, 0, 1], [(8, 8), SHAPES[0], SHAPES[2]])


def edge_dz_ulp_case():
    """max_edge_dz = 0.5 on a 5 x 4 map at 4 m with one vertex exactly 0.5 m behind (its triangles stay: the comparison
    is strict) and another one float32 ulp further than that (its six triangles go, and so does it)."""
    z = np.full((5, 4), 4.0)
    z[1, 1] = 4.5
    z[3, 2] = np.float64(np.nextafter(np.float32(4.5), np.float32(np.inf)))
    rows, cols = np.meshgrid(1 + np.arange(5), 1 + np.arange(4), indexing='ij')
    return _case([at_pixels(cols, rows, z)], [0], [SHAPES[1]], max_edge_dz=0.5)


_OWN = {'spike_3x3': spike_case, 'hidden_box': hidden_case, 'edge_dz_ulp_5x4': edge_dz_ulp_case}
# from tests/surface_cases.py: the smallest maps, masks and keep flags that leave holes (invalid_vertices, the random
# ones: three frames, the middle one without a box), max_edge_dz and max_span_px met and exceeded by one, zero-area and
# folded maps, identical boxes, vertices off the image, and 48 x 48 maps on 96 x 128 pixels
SHARED = ('cell_2x2', 'fractional_2x3', 'mirrored_4x5', 'invalid_vertices', 'edge_dz', 'span_limit', 'degenerate',
          'identical_boxes', 'off_image', 'random_b12_5x4', 'random_b3_2x3', 'big_48x48')
NAMES = SHARED + tuple(_OWN)
# the cases whose boxes hold no two points with the same coordinates: a vertex's map point follows from its xyz
DISTINCT_POINTS = tuple(n for n in NAMES if n != 'degenerate')
DETERMINISM_CASES = ('random_b12_5x4', 'big_48x48')


@functools.lru_cache(maxsize=None)
def case(name):
    return _OWN[name]() if name in _OWN else surface_cases.case(name)


@functools.lru_cache(maxsize=None)
def rendering(name):
    return surface_cases.expected(name) if name in SHARED else mesh_restatement.surface_restatement.render(case(name))


@functools.lru_cache(maxsize=None)
def images(name):
    """One (h, w, 3) float32 image per frame: seeded values in [0, 255) off the integers."""
    rng = np.random.default_rng(9000 + NAMES.index(name))
    return tuple(rng.uniform(0.0, 255.0, (int(h), int(w), 3)).astype(np.float32) for h, w in case(name)['shapes'])


@functools.lru_cache(maxsize=None)
def expected(name, visible_only, with_images=True):
    return mesh_restatement.mesh(case(name), rendering(name), visible_only, images(name) if with_images else None)
