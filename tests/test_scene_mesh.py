"""Surfaces as meshes without a GPU: the two entry points' declarations and host-side argument
checks, the mesh PLY files, the command line's flags, and the properties the restatement of tests/mesh_restatement.py
must have by itself."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import mesh_cases as cases
import mesh_restatement as restatement
import surface_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ('mpsr_scene_surface_mesh_workspace_bytes', 'mpsr_scene_surface_mesh')


def test_new_names_are_declared_bound_and_exported():
    import subprocess
    from monopsr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'monopsr_hip.h')).read()
    exported = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    lib = _lib.lib()
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert re.search(r' T %s\b' % name, exported), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.ABI_VERSION == 13 and lib.mpsr_abi_version() == 13
    # the render workspace is what it was
    assert lib.mpsr_scene_surface_workspace_bytes(2, 99, 3, 48, 48) == 1024 + 3 * 48 * 48 * 8 + 256 + 256 + 256


def _mesh(lib, nf, nb, mh, mw, dz=1.0, span=64, visible=0, ptr=None, host_bf=None, host_hw=None, host_offs=None,
          rws=(None, 0), mws=(None, 0), **null):
    """mpsr_scene_surface_mesh with `ptr` for every device pointer (never dereferenced: each call fails or returns on
    the host) and the host tables where given."""
    a = dict(xyz_in=ptr, box_frame=ptr, box_frame_host=host_bf, cam=ptr, hw=ptr, hw_host=host_hw, offs=ptr,
             offs_host=host_offs, images=None, xyz=ptr, rgb=ptr, normal=ptr, vertex_box=ptr, faces=ptr, face_box=ptr,
             area=ptr, v_box=ptr, v_frame=ptr, t_box=ptr, t_frame=ptr)
    a.update(null)
    return lib.mpsr_scene_surface_mesh(
        a['xyz_in'], a['box_frame'], a['box_frame_host'], a['cam'], a['hw'], a['hw_host'], a['offs'], a['offs_host'],
        a['images'], nf, nb, mh, mw, dz, span, visible, rws[0], rws[1], mws[0], mws[1], a['xyz'], a['rgb'],
        a['normal'], a['vertex_box'], a['faces'], a['face_box'], a['area'], a['v_box'], a['v_frame'], a['t_box'],
        a['t_frame'], None)


def test_host_checks_of_the_entry_points_need_no_gpu():
    from monopsr_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(256)
    as_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bf = np.ascontiguousarray(np.asarray([0, 1, 1], np.int32))
    hw = np.ascontiguousarray(np.asarray([[5, 7], [8, 8]], np.int32))
    offs = np.ascontiguousarray(np.asarray([0, 35, 99], np.int64))
    tables = dict(ptr=fake, host_bf=as_ptr(bf), host_hw=as_ptr(hw), host_offs=as_ptr(offs))
    wsb = lib.mpsr_scene_surface_mesh_workspace_bytes
    # the workspace size: a byte per triangle, an int per point, two ints per box, each region aligned to 256 bytes
    assert wsb(3, 48, 48) == 13312 + 3 * 48 * 48 * 4 + 256 + 256  # 3 * 2 * 47 * 47 = 13254 bytes -> 13312
    assert wsb(1, 2, 2) == 4 * 256
    assert wsb(0, 4, 4) == 0 and wsb(3, 1, 4) == 0 and wsb(3, 4, 1) == 0 and wsb(-1, 4, 4) == 0
    assert wsb(1 << 30, 3, 3) == 0 and wsb(1 << 15, 257, 257) == 0  # points beyond INT_MAX, triangle ids beyond 2^32
    render_need = lib.mpsr_scene_surface_workspace_bytes(2, 99, 3, 4, 4)
    need = wsb(3, 4, 4)
    # the map: 2 x 2 or more, before anything else (even with empty sizes)
    for mh, mw in ((1, 4), (4, 1), (0, 0), (-3, 4)):
        assert _mesh(lib, 2, 3, mh, mw, **tables) == 1 and b'map_h and map_w must be 2 or more' in lib.mpsr_last_error()
        assert _mesh(lib, 0, 0, mh, mw) == 1
    for span in (0, 1025, -1):
        assert _mesh(lib, 2, 3, 4, 4, span=span, **tables) == 1 and b'max_span_px' in lib.mpsr_last_error()
    for dz in (0.0, -1.0, float('nan'), -float('inf')):
        assert _mesh(lib, 2, 3, 4, 4, dz=dz, **tables) == 1 and b'max_edge_dz' in lib.mpsr_last_error()
    assert _mesh(lib, 2, 3, 4, 4, dz=float('inf'), span=1, **tables) == 3 and b'workspace' in lib.mpsr_last_error()
    assert _mesh(lib, 2, 3, 4, 4, dz=1e-30, span=1024, **tables) == 3
    # the triangle id must fit 32 bits, a vertex index 31
    assert _mesh(lib, 1, 1 << 15, 257, 257, **tables) == 1 and b'32 bits' in lib.mpsr_last_error()
    assert _mesh(lib, 1, 1 << 30, 3, 2) == 1 and b'32 bits' in lib.mpsr_last_error()
    assert _mesh(lib, 1, 1 << 28, 3, 3, **tables) == 1 and b'31 bits' in lib.mpsr_last_error()
    # empty sizes succeed (null offset tables are left alone: nothing is launched); negative ones do not
    nothing = dict(v_box=None, v_frame=None, t_box=None, t_frame=None)
    assert _mesh(lib, 0, 3, 4, 4, **nothing) == 0 and _mesh(lib, 2, 0, 4, 4, **nothing) == 0
    assert _mesh(lib, -1, 3, 4, 4) == 1 and b'negative' in lib.mpsr_last_error()
    # null pointers with non-empty sizes: inputs, outputs, offset tables
    full = dict(tables, rws=(fake, render_need), mws=(fake, need))
    for key in ('xyz_in', 'box_frame', 'box_frame_host', 'cam', 'hw', 'hw_host', 'offs', 'offs_host', 'xyz', 'rgb',
                'normal', 'vertex_box', 'faces', 'face_box', 'area', 'v_box', 'v_frame', 't_box', 't_frame'):
        assert _mesh(lib, 2, 3, 4, 4, **dict(full, **{key: None})) == 1, key
        assert b'null' in lib.mpsr_last_error(), key
    # the frame tables
    bad = np.ascontiguousarray(np.asarray([0, 35, 98], np.int64))
    assert _mesh(lib, 2, 3, 4, 4, **dict(full, host_offs=as_ptr(bad))) == 1 and b'spans' in lib.mpsr_last_error()
    for frames, what in (([0, 2, 1], b'of frame 2'), ([1, 0, 1], b'decreases')):
        b = np.ascontiguousarray(np.asarray(frames, np.int32))
        assert _mesh(lib, 2, 3, 4, 4, **dict(full, host_bf=as_ptr(b))) == 1 and what in lib.mpsr_last_error()
    # either workspace missing or short: status 3, still before any launch
    for rws, mws in (((None, 0), (fake, need)), ((fake, render_need - 1), (fake, need)),
                     ((fake, render_need), (None, 0)), ((fake, render_need), (fake, need - 1))):
        assert _mesh(lib, 2, 3, 4, 4, **dict(tables, rws=rws, mws=mws)) == 3 and b'workspace' in lib.mpsr_last_error()


# ---- files


def _generic_ply(path):
    """A small PLY reader that knows the format, not the writer: the header's elements and properties make the layout.
    -> {element: {property: array}}; a list property becomes an (n, k) array (all lists of one length k)."""
    scalar = {'char': 'i1', 'uchar': 'u1', 'short': '<i2', 'ushort': '<u2', 'int': '<i4', 'uint': '<u4',
              'float': '<f4', 'double': '<f8'}
    data = open(path, 'rb').read()
    head, body = data.split(b'end_header\n', 1)
    lines = head.decode('ascii').splitlines()
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    elements = []
    for line in lines[2:]:
        words = line.split()
        if words[0] == 'element':
            elements.append((words[1], int(words[2]), []))
        elif words[0] == 'property':
            elements[-1][2].append(words[1:])
        else:
            assert words[0] == 'comment', line
    out, at = {}, 0
    for name, n, props in elements:
        if any(p[0] == 'list' for p in props):
            assert len(props) == 1
            _, count_type, item_type, prop = props[0]
            rows = []
            for _ in range(n):
                k = int(np.frombuffer(body, scalar[count_type], 1, at)[0])
                at += np.dtype(scalar[count_type]).itemsize
                rows.append(np.frombuffer(body, scalar[item_type], k, at))
                at += k * np.dtype(scalar[item_type]).itemsize
            out[name] = {prop: np.asarray(rows).reshape(n, -1) if n else np.zeros((0, 0), scalar[item_type])}
        else:
            dtype = np.dtype([(p[1], scalar[p[0]]) for p in props])
            rec = np.frombuffer(body, dtype, n, at)
            at += n * dtype.itemsize
            out[name] = {p[1]: rec[p[1]] for p in props}
    assert at == len(body)
    return out


def test_mesh_ply_round_trip_and_a_generic_reader(tmp_path):
    from monopsr_amd.core import scene_reconstruction as sr
    rng = np.random.default_rng(3)
    n, t = 11, 7
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    normal = rng.normal(size=(n, 3)).astype(np.float32)
    rgb = np.concatenate([rng.uniform(-20.0, 300.0, (n - 3, 3)), [[254.5, 255.5, -0.5], [0.5, 1.5, np.nan],
                                                                  [2.5, 300.0, 127.49]]]).astype(np.float32)
    box = rng.integers(0, 5, n).astype(np.int32)
    faces = rng.integers(0, n, (t, 3)).astype(np.int32)
    path = str(tmp_path / 'mesh.ply')
    sr.write_mesh_ply(path, xyz, faces, rgb, normal, box)
    got = sr.read_mesh_ply(path)
    assert [a.dtype for a in got] == [np.float32, np.int32, np.uint8, np.float32, np.int32]
    assert got[0].tobytes() == xyz.tobytes() and np.array_equal(got[1], faces) and got[3].tobytes() == normal.tobytes()
    assert np.array_equal(got[2], sr.colours_to_uint8(rgb)) and np.array_equal(got[4], box)
    assert got[2][-3:].tolist() == [[254, 255, 0], [0, 2, 0], [2, 255, 127]]
    assert os.path.getsize(path) == len(sr._MESH_HEADER % (n, t)) + n * 31 + t * 13
    generic = _generic_ply(path)
    assert list(generic) == ['vertex', 'face']
    assert list(generic['vertex']) == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue', 'box']
    v = generic['vertex']
    assert np.array_equal(np.stack([v['x'], v['y'], v['z']], 1).view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(np.stack([v['nx'], v['ny'], v['nz']], 1).view(np.uint32), normal.view(np.uint32))
    assert np.array_equal(np.stack([v['red'], v['green'], v['blue']], 1), got[2]) and np.array_equal(v['box'], box)
    assert np.array_equal(generic['face']['vertex_indices'], faces)
    # uint8 colours go through as they are; the optional columns default to 0; 0 vertices and 0 faces
    sr.write_mesh_ply(path, xyz, faces, got[2])
    again = sr.read_mesh_ply(path)
    assert np.array_equal(again[2], got[2]) and not again[3].any() and not again[4].any()
    sr.write_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    empty = sr.read_mesh_ply(path)
    assert [a.shape for a in empty] == [(0, 3), (0, 3), (0, 3), (0, 3), (0,)]
    assert _generic_ply(path)['face']['vertex_indices'].shape[0] == 0
    dirs = sr.mesh_output_dirs(str(tmp_path / 'out'))
    assert sr.MESH_DIRS == ('mesh',) and list(dirs) == ['mesh'] and os.path.isdir(dirs['mesh'])
    saved = sr.save_empty_mesh_frame(dirs, '000007')
    assert saved == os.path.join(dirs['mesh'], '000007.ply') and sr.read_mesh_ply(saved)[0].shape == (0, 3)
    # an index outside the vertices is refused; so is a file cut short; and read_ply takes no mesh file, nor
    # read_mesh_ply a point file
    with pytest.raises(ValueError):
        sr.write_mesh_ply(path, xyz, np.asarray([[0, 1, n]]))
    sr.write_mesh_ply(path, xyz, faces, rgb, normal, box)
    with pytest.raises(ValueError):
        sr.read_ply(path)
    data = open(path, 'rb').read()
    open(path, 'wb').write(data[:-1])
    with pytest.raises(ValueError):
        sr.read_mesh_ply(path)
    points = str(tmp_path / 'points.ply')
    sr.write_ply(points, xyz, rgb, box)
    assert sr.read_ply(points)[0].tobytes() == xyz.tobytes()
    with pytest.raises(ValueError):
        sr.read_mesh_ply(points)


def test_run_inference_accepts_meshes():
    from monopsr_amd.experiments import run_inference
    need = ['cfg.yaml', 'ckpt', '--mscnn-dir', 'm', '--output-dir', 'o']
    ap = run_inference.build_parser()
    plain = run_inference.parse_args(ap, need)
    assert plain.meshes is False and plain.mesh_visible_only is False and plain.surfaces is False
    assert run_inference.surface_options(plain) is None
    surfaces = run_inference.parse_args(ap, need + ['--surfaces'])
    assert run_inference.surface_options(surfaces) == dict(max_edge_dz=1.0, max_span_px=64)
    args = run_inference.parse_args(ap, need + ['--meshes', '--max-edge-dz', '0.5', '--max-span-px', '128'])
    assert args.meshes is True and args.surfaces is True  # --meshes implies --surfaces
    assert run_inference.surface_options(args) == dict(max_edge_dz=0.5, max_span_px=128, mesh=True, mesh_visible_only=False)
    args = run_inference.parse_args(ap, need + ['--meshes', '--mesh-visible-only', '--min-score', '0.3', '--fit-centroids'])
    assert run_inference.surface_options(args)['mesh_visible_only'] is True and args.min_score == 0.3 and args.fit_centroids
    with pytest.raises(SystemExit):
        run_inference.parse_args(ap, need + ['--mesh-visible-only'])
    writer = run_inference.SceneWriter(None, 'base', surfaces=run_inference.surface_options(args))
    assert writer.meshes is True and run_inference.SceneWriter(None, 'base', surfaces={}).meshes is False
    assert run_inference.SceneWriter(None, 'base').meshes is False


# ---- properties of the restatement itself


def _full_grid(mh, mw, **kw):
    return surface_cases._case([surface_cases.plane(1, 1, 1, 1, mh, mw)], [0], [(mh + 2, mw + 2)], **kw)


def test_full_grid_counts():
    for mh, mw in ((2, 2), (2, 3), (5, 4), (9, 7)):
        m = restatement.mesh(_full_grid(mh, mw))
        assert len(m['xyz']) == mh * mw and len(m['faces']) == 2 * (mh - 1) * (mw - 1)
        assert m['point'].tolist() == list(range(mh * mw)) and m['tri'].tolist() == list(range(len(m['faces'])))
        assert m['vertex_box_offset'].tolist() == [0, mh * mw] == m['vertex_frame_offset'].tolist()
        assert m['face_box_offset'].tolist() == [0, len(m['faces'])] == m['face_frame_offset'].tolist()
        # k = 0: (v00, v10, v01); k = 1: (v11, v01, v10)
        assert m['faces'][0].tolist() == [0, mw, 1] and m['faces'][1].tolist() == [mw + 1, 1, mw]


@pytest.mark.parametrize('name', cases.NAMES)
def test_every_edge_is_shared_by_at_most_two_faces_in_opposite_directions(name):
    for visible_only in (False, True):
        m = cases.expected(name, visible_only)
        nf = len(m['vertex_frame_offset']) - 1
        for f in range(nf):
            v = int(m['vertex_frame_offset'][f + 1] - m['vertex_frame_offset'][f])
            faces = m['faces'][int(m['face_frame_offset'][f]):int(m['face_frame_offset'][f + 1])]
            boxes = m['face_box'][int(m['face_frame_offset'][f]):int(m['face_frame_offset'][f + 1])]
            assert faces.size == 0 or (0 <= int(faces.min()) and int(faces.max()) < v)
            directed = set()
            for (a, b, c), box in zip(faces.tolist(), boxes.tolist()):
                for edge in ((a, b), (b, c), (c, a)):
                    assert edge not in directed, (name, f, edge)  # a second face along an edge runs the other way
                    directed.add(edge)
                # a face stays inside its own box
                lo = int(m['vertex_box_offset'][box] - m['vertex_frame_offset'][f])
                hi = int(m['vertex_box_offset'][box + 1] - m['vertex_frame_offset'][f])
                assert lo <= min(a, b, c) and max(a, b, c) < hi
            # every vertex is used by a face
            assert sorted(set(faces.reshape(-1).tolist())) == list(range(v))


def test_fronto_parallel_normals_and_the_fold():
    m = restatement.mesh(surface_cases.case('on_centres_4x5'))
    assert len(m['normal']) == 20 and np.array_equal(m['normal'], np.tile(np.float32([0.0, 0.0, -1.0]), (20, 1)))
    # the same surface with its columns reversed faces away from the camera: the normals flip, the face order does not
    flipped = restatement.mesh(surface_cases.case('mirrored_4x5'))
    assert np.array_equal(flipped['normal'][:, 2], np.ones(20, np.float32)) and not flipped['normal'][:, :2].any()
    assert np.array_equal(flipped['faces'], m['faces'])
    # the folded 3 x 4 map of the degenerate case: its middle cells face away, the outer ones toward the camera
    fold = cases.expected('degenerate', False)
    v = fold['xyz'][int(fold['vertex_box_offset'][1]):int(fold['vertex_box_offset'][2])].astype(np.float64)
    tri = fold['faces'][int(fold['face_box_offset'][1]):int(fold['face_box_offset'][2])]  # (one box per frame)
    z = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])[:, 2]
    assert len(z) == 12 and int((z < 0).sum()) == 8 and int((z > 0).sum()) == 4
    # a vertex whose triangles cancel, or with no area at all, has the normal (0, 0, 0): box 0 of that case has no face
    assert int(fold['vertex_box_offset'][1]) == 0 and fold['area'][0] == 0.0


def test_area_of_a_planar_rectangle():
    """A 6 x 9 grid with cells of 0.3 m x 0.7 m in the plane z = 5: the analytic area is 5 * 8 * 0.21 m^2.  The bound:
    a coordinate is rounded to float32 with a relative error of at most 2^-24, so by d = 2^-24 max |coordinate| at the
    most; an edge vector u = c - a or v = b - a moves by at most 2 d per component, in x and y only (z = 5 is exact),
    so |du|, |dv| <= 2 sqrt(2) d; a triangle's area 0.5 |u x v| moves by at most 0.5 (|du| |v| + |u| |dv| + |du| |dv|);
    the fp64 arithmetic itself (differences exact to 2^-53, some twenty operations per triangle and the sums) is
    allowed a relative 1e-13 on top."""
    mh, mw, ex, ey = 6, 9, 0.3, 0.7
    i, j = np.meshgrid(np.arange(mh), np.arange(mw), indexing='ij')
    xyz = np.stack([-1.1 + ex * j, -2.3 + ey * i, np.full(i.shape, 5.0)], -1).astype(np.float32)
    cam = surface_cases.scene_cases.pow2_camera(4.0, 8.0, 8.0)
    case = dict(xyz=xyz[None], box_frame=np.zeros(1, np.int64), cam_p=cam[None], shapes=[(16, 16)])
    m = restatement.mesh(case)
    n_tris = 2 * (mh - 1) * (mw - 1)
    assert len(m['faces']) == n_tris
    exact = (mh - 1) * (mw - 1) * ex * ey
    d = 2.0 ** -24 * float(np.abs(xyz).max())
    du = 2.0 * math.sqrt(2.0) * d
    bound = n_tris * 0.5 * (du * ex + ey * du + du * du) + 1e-13 * exact
    assert abs(float(m['area'][0]) - exact) <= bound, (float(m['area'][0]), exact, bound)
    assert bound < 1e-5 * exact  # the bound is one worth having
    # and the exact case: powers of two throughout
    flat = restatement.mesh(_full_grid(5, 4))
    assert flat['area'][0] == 4.0 * 3.0  # vertices one pixel apart at z = 4, f = 4: 1 m apart


def test_vertices_and_colours_of_the_small_cases():
    # the vertex whose six triangles are all dropped is no vertex, nor are the two corners that hang on it
    spike = cases.expected('spike_3x3', False)
    assert spike['point'][:6].tolist() == [0, 1, 3, 5, 7, 8] and spike['tri'][:2].tolist() == [0, 7]
    assert spike['vertex_frame_offset'].tolist() == [0, 15, 15, 15] and spike['face_frame_offset'].tolist() == [0, 10, 10, 10]
    # max_edge_dz met (kept) and exceeded by one ulp (six triangles and the vertex go)
    edge = cases.expected('edge_dz_ulp_5x4', False)
    assert len(edge['xyz']) == 19 and 3 * 4 + 2 not in edge['point'].tolist() and 1 * 4 + 1 in edge['point'].tolist()
    assert len(edge['faces']) == 2 * 4 * 3 - 6
    # span_limit's boxes: an extent of max_span_px is a mesh, one more is none
    span = cases.expected('span_limit', False)
    per_box = np.diff(span['face_box_offset'])
    assert per_box.tolist() == [2 if kind[-1] else 0 for kind in surface_cases.SPAN_KINDS]
    # a box wholly hidden: no face, no vertex with visible_only, and the next box goes on from there
    hidden = cases.expected('hidden_box', True)
    assert hidden['vertex_box_offset'].tolist() == [0, 0, 9, 18] and hidden['face_box_offset'].tolist() == [0, 0, 8, 16]
    assert hidden['area'][0] == 0.0 and hidden['faces'][:8].max() < 9 and hidden['faces'][8:].max() < 9
    # identical boxes: the lower triangle ids keep the shared pixels
    same = cases.expected('identical_boxes', True)
    assert np.diff(same['face_box_offset']).tolist()[:2] == [8, 0]
    # off-image vertices are kept and black; the others have their pixel's colour
    off = cases.expected('off_image', False)
    case, images = cases.case('off_image'), cases.images('off_image')
    assert len(off['xyz']) == 6 * 12
    black = ~off['rgb'].any(1)
    assert bool(black.any()) and bool((~black).any())
    for v in range(len(off['xyz'])):
        x, y, z = (float(c) for c in off['xyz'][v])
        col, row = 4.0 * x / z, 4.0 * y / z  # pow2_camera(4, 0, 0); exact in this case
        inside = 0 <= round(col) < 7 and 0 <= round(row) < 5
        assert inside != bool(black[v]), v
        if inside and col == int(col) and row == int(row):
            assert np.array_equal(off['rgb'][v], images[0][int(row), int(col)])
    assert not cases.expected('off_image', False, with_images=False)['rgb'].any()
    # xyz is the input, bit for bit, at the vertex's point
    for name in cases.NAMES:
        m = cases.expected(name, False)
        flat = np.asarray(cases.case(name)['xyz'], np.float32).reshape(-1, 3)
        assert np.array_equal(m['xyz'].view(np.uint32), flat[m['point']].view(np.uint32)), name
