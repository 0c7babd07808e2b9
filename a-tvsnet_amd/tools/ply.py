"""Binary PLY point clouds in the layout the reference's fusibile writes (fusibile/displayUtils.h:80-135):
`format binary_little_endian 1.0`, vertices of (float x, y, z, uchar red, green, blue); with normals (not in the reference)
(float x, y, z, nx, ny, nz, uchar red, green, blue).  Triangle meshes (write_mesh / read_mesh / read_mesh_normals): either vertex
element followed by `element face` with `property list uchar int vertex_indices`."""
import numpy as np

_VERTEX = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')])


_VERTEX_N = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4'),
                      ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')])
_HEADER_TYPES = {'f4': 'float', 'u1': 'uchar'}
_FACE = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])


def write_ply(path, points, colors, normals=None):
    """points (M,3) float32, colors (M,3) uint8 (r, g, b).  Non-finite coordinates are written as (0,0,0) like the
    reference (:115-119).  normals (M,3) float32: the vertex becomes (x, y, z, nx, ny, nz, red, green, blue); a non-finite
    normal is written as (0,0,0)."""
    points = np.asarray(points, np.float32).reshape(-1, 3).copy()
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    bad = ~np.isfinite(points).all(axis=1)
    points[bad] = 0.0
    v = np.empty(len(points), _VERTEX if normals is None else _VERTEX_N)
    v['x'], v['y'], v['z'] = points[:, 0], points[:, 1], points[:, 2]
    v['red'], v['green'], v['blue'] = colors[:, 0], colors[:, 1], colors[:, 2]
    if normals is not None:
        normals = np.asarray(normals, np.float32).reshape(-1, 3).copy()
        if len(normals) != len(points):
            raise ValueError('write_ply: %d normals for %d points' % (len(normals), len(points)))
        normals[~np.isfinite(normals).all(axis=1)] = 0.0
        v['nx'], v['ny'], v['nz'] = normals[:, 0], normals[:, 1], normals[:, 2]
    with open(path, 'wb') as f:
        f.write(('ply\nformat binary_little_endian 1.0\nelement vertex %d\n' % len(points)).encode('ascii'))
        f.write(''.join('property %s %s\n' % (_HEADER_TYPES[v.dtype[name].str[1:]], name) for name in v.dtype.names).encode('ascii'))
        f.write(b'end_header\n')
        v.tofile(f)


def _header(f, path):
    """The header of an open file -> (vertex count or None, the vertex element's property names in order: the properties of a
    later element, a mesh's faces, are not collected); the file is left at the body."""
    n, names, element = None, [], None
    while True:
        raw = f.readline()
        if not raw:
            raise ValueError('%s: the header has no end_header' % path)
        line = raw.decode('ascii').strip()
        if line.startswith('element'):
            element = line.split()[1] if len(line.split()) > 1 else None
        if line.startswith('element vertex'):
            n = int(line.split()[-1])
        if line.startswith('property') and element in (None, 'vertex'):
            names.append(line.split()[-1])
        if line == 'end_header':
            return n, names


def has_normals(path):
    """Whether read_ply_normals would return normals for this file: its header alone is read."""
    with open(path, 'rb') as f:
        return tuple(_header(f, path)[1]) == _VERTEX_N.names


def read_ply_normals(path):
    """-> (points (M,3) float32, colors (M,3) uint8, normals (M,3) float32 or None) of a file written by write_ply / the reference,
    by the vertex properties its header lists: with or without nx, ny, nz."""
    with open(path, 'rb') as f:
        n, names = _header(f, path)
        layout = {_VERTEX.names: _VERTEX, _VERTEX_N.names: _VERTEX_N}.get(tuple(names))
        if layout is None or n is None:
            raise ValueError('%s: not a vertex layout write_ply writes: %s' % (path, ' '.join(names)))
        v = np.fromfile(f, layout, n)
    normals = np.stack([v['nx'], v['ny'], v['nz']], -1) if layout is _VERTEX_N else None
    return np.stack([v['x'], v['y'], v['z']], -1), np.stack([v['red'], v['green'], v['blue']], -1), normals


def read_ply(path):
    """-> (points (M,3) float32, colors (M,3) uint8) of a file written by write_ply / the reference (with or without normals)."""
    return read_ply_normals(path)[:2]


def write_mesh(path, vertices, colors, faces, normals=None):
    """vertices (V,3) float32, colors (V,3) uint8 (r, g, b) or None (white), faces (F,3) int32 -> a binary little-endian PLY:
    `element vertex` as write_ply writes it (x y z red green blue; with normals (V,3) float32 x y z nx ny nz red green blue, a
    non-finite normal as (0,0,0)), then `element face` with `property list uchar int vertex_indices`.  A face index outside the
    vertices raises."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    if colors is None:
        colors = np.full((len(vertices), 3), 255, np.uint8)
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    if len(colors) != len(vertices):
        raise ValueError('write_mesh: %d colors for %d vertices' % (len(colors), len(vertices)))
    if len(faces) and (faces.min() < 0 or faces.max() >= len(vertices)):
        raise ValueError('write_mesh: a face index outside 0..%d' % (len(vertices) - 1))
    v = np.empty(len(vertices), _VERTEX if normals is None else _VERTEX_N)
    v['x'], v['y'], v['z'] = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    v['red'], v['green'], v['blue'] = colors[:, 0], colors[:, 1], colors[:, 2]
    if normals is not None:
        normals = np.asarray(normals, np.float32).reshape(-1, 3).copy()
        if len(normals) != len(vertices):
            raise ValueError('write_mesh: %d normals for %d vertices' % (len(normals), len(vertices)))
        normals[~np.isfinite(normals).all(axis=1)] = 0.0
        v['nx'], v['ny'], v['nz'] = normals[:, 0], normals[:, 1], normals[:, 2]
    t = np.empty(len(faces), _FACE)
    t['n'] = 3
    t['v'] = faces
    with open(path, 'wb') as f:
        f.write(('ply\nformat binary_little_endian 1.0\nelement vertex %d\n' % len(vertices)).encode('ascii'))
        f.write(''.join('property %s %s\n' % (_HEADER_TYPES[v.dtype[name].str[1:]], name) for name in v.dtype.names).encode('ascii'))
        f.write(('element face %d\nproperty list uchar int vertex_indices\nend_header\n' % len(faces)).encode('ascii'))
        v.tofile(f)
        t.tofile(f)


def read_mesh_normals(path):
    """-> (vertices (V,3) float32, colors (V,3) uint8, faces (F,3) int32, normals (V,3) float32 or None) of a file written by
    write_mesh, by the vertex properties its header lists: with or without nx, ny, nz."""
    with open(path, 'rb') as f:
        lines = []
        while not lines or lines[-1] != 'end_header':
            raw = f.readline()
            if not raw:
                raise ValueError('%s: the header has no end_header' % path)
            lines.append(raw.decode('ascii').strip())
        elements = [ln.split() for ln in lines if ln.startswith('element')]
        props = [ln for ln in lines if ln.startswith('property')]
        layout = {_VERTEX.names: _VERTEX, _VERTEX_N.names: _VERTEX_N}.get(tuple(p.split()[-1] for p in props[:-1]))
        if ([e[1] for e in elements] != ['vertex', 'face'] or lines[1] != 'format binary_little_endian 1.0' or layout is None or
                props[-1] != 'property list uchar int vertex_indices'):
            raise ValueError('%s: not a mesh layout write_mesh writes' % path)
        nv, nf = int(elements[0][2]), int(elements[1][2])
        v = np.fromfile(f, layout, nv)
        t = np.fromfile(f, _FACE, nf)
    if len(v) != nv or len(t) != nf or (nf and (t['n'] != 3).any()):
        raise ValueError('%s: truncated body, or a face that is no triangle' % path)
    normals = np.stack([v['nx'], v['ny'], v['nz']], -1).reshape(-1, 3) if layout is _VERTEX_N else None
    return (np.stack([v['x'], v['y'], v['z']], -1).reshape(-1, 3), np.stack([v['red'], v['green'], v['blue']], -1).reshape(-1, 3),
            t['v'].astype(np.int32).reshape(-1, 3), normals)


def read_mesh(path):
    """-> (vertices (V,3) float32, colors (V,3) uint8, faces (F,3) int32) of a file written by write_mesh (with or without normals)."""
    return read_mesh_normals(path)[:3]


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def read_ply_points(path):
    """-> points (M,3) float32 of any PLY's `vertex` element: `ascii`, `binary_little_endian` or `binary_big_endian`; x, y, z as
    `float` or `double` (a double is rounded once to float32) at any position among other scalar properties; elements after
    `vertex` (faces) are ignored.  A list property inside `vertex`, an element in front of it, a missing coordinate, a malformed
    header or a truncated body raises ValueError naming the file."""
    def bad(why):
        return ValueError('%s: %s' % (path, why))

    with open(path, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise bad('not a PLY file (no "ply" magic)')
        fmt, count, props, element = None, None, [], None
        while True:
            raw = f.readline()
            if not raw:
                raise bad('the header has no end_header')
            words = raw.decode('ascii', 'replace').split()
            if not words or words[0] in ('comment', 'obj_info'):
                continue
            if words[0] == 'end_header':
                break
            if words[0] == 'format' and len(words) >= 2:
                fmt = words[1]
            elif words[0] == 'element' and len(words) == 3:
                element = words[1]
                if element == 'vertex':
                    try:
                        count = int(words[2])
                    except ValueError:
                        raise bad('element vertex: bad count %r' % words[2])
                elif count is None:
                    raise bad('element %r in front of the vertex element is not supported' % element)
            elif words[0] == 'property' and element == 'vertex':
                if len(words) >= 2 and words[1] == 'list':
                    raise bad('a list property inside the vertex element is not supported')
                if len(words) != 3 or words[1] not in _PLY_TYPES:
                    raise bad('bad property line %r' % ' '.join(words))
                props.append((words[2], _PLY_TYPES[words[1]]))
        if fmt not in ('ascii', 'binary_little_endian', 'binary_big_endian'):
            raise bad('unsupported format %r' % fmt)
        if count is None or count < 0:
            raise bad('no vertex element')
        names = [p[0] for p in props]
        for c in 'xyz':
            if names.count(c) != 1:
                raise bad('the vertex element has no (single) property %r' % c)
            if dict(props)[c] not in ('f4', 'f8'):
                raise bad('property %r is neither float nor double' % c)
        if fmt == 'ascii':
            cols = [names.index(c) for c in 'xyz']
            out = np.empty((count, 3), np.float64)
            for i in range(count):
                words = f.readline().split()
                if len(words) < len(props):
                    raise bad('truncated body: vertex %d of %d' % (i, count))
                try:
                    out[i] = [float(words[c]) for c in cols]
                except ValueError:
                    raise bad('vertex %d: not a number' % i)
            return out.astype(np.float32)
        order = '<' if fmt == 'binary_little_endian' else '>'
        dtype = np.dtype([(n, order + t) for n, t in props])
        body = f.read(count * dtype.itemsize)
        if len(body) != count * dtype.itemsize:
            raise bad('truncated body: %d bytes for %d vertices of %d bytes' % (len(body), count, dtype.itemsize))
        v = np.frombuffer(body, dtype, count)
        return np.stack([v['x'].astype(np.float32), v['y'].astype(np.float32), v['z'].astype(np.float32)], -1).reshape(count, 3)


def read_mesh_any(path):
    """-> (vertices (V,3) float32, faces (F,3) int32) of a third-party triangle-mesh PLY: `ascii`, `binary_little_endian` or
    `binary_big_endian`; a `vertex` element with x, y, z as `float` or `double` among other scalar properties (skipped), then a
    `face` element with one list property `vertex_indices` or `vertex_index`, its count and its indices of any integer type, among
    other scalar properties (skipped); later elements are ignored.  A polygon with more than three corners (or fewer), any other
    layout, a malformed header or a truncated body raises ValueError naming the file."""
    def bad(why):
        return ValueError('%s: %s' % (path, why))

    with open(path, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise bad('not a PLY file (no "ply" magic)')
        fmt, elements = None, []
        while True:
            raw = f.readline()
            if not raw:
                raise bad('the header has no end_header')
            words = raw.decode('ascii', 'replace').split()
            if not words or words[0] in ('comment', 'obj_info'):
                continue
            if words[0] == 'end_header':
                break
            if words[0] == 'format' and len(words) >= 2:
                fmt = words[1]
            elif words[0] == 'element' and len(words) == 3 and words[2].isdigit():
                elements.append((words[1], int(words[2]), []))
            elif words[0] == 'property' and elements:
                if len(words) == 5 and words[1] == 'list' and words[2] in _PLY_TYPES and words[3] in _PLY_TYPES:
                    elements[-1][2].append((words[4], _PLY_TYPES[words[2]], _PLY_TYPES[words[3]]))
                elif len(words) == 3 and words[1] in _PLY_TYPES:
                    elements[-1][2].append((words[2], _PLY_TYPES[words[1]], None))
                else:
                    raise bad('bad property line %r' % ' '.join(words))
            else:
                raise bad('bad header line %r' % ' '.join(words))
        if fmt not in ('ascii', 'binary_little_endian', 'binary_big_endian'):
            raise bad('unsupported format %r' % fmt)
        if [e[0] for e in elements[:2]] != ['vertex', 'face']:
            raise bad('expected a vertex element and then a face element, got %s' % [e[0] for e in elements])
        (_, nv, vprops), (_, nf, fprops) = elements[:2]
        vnames = [p[0] for p in vprops]
        if any(p[2] is not None for p in vprops):
            raise bad('a list property inside the vertex element is not supported')
        for c in 'xyz':
            if vnames.count(c) != 1 or vprops[vnames.index(c)][1] not in ('f4', 'f8'):
                raise bad('the vertex element has no (single) float or double property %r' % c)
        lists = [k for k, p in enumerate(fprops) if p[2] is not None]
        if len(lists) != 1 or fprops[lists[0]][0] not in ('vertex_indices', 'vertex_index'):
            raise bad('the face element needs exactly one list property, vertex_indices or vertex_index')
        li = lists[0]
        if fprops[li][1][0] not in 'iu' or fprops[li][2][0] not in 'iu':
            raise bad('the face list\'s count and indices must be integers')

        def polygon(i, n):
            return bad('face %d is a polygon with %d corners: triangles only' % (i, n))
        if fmt == 'ascii':
            cols = [vnames.index(c) for c in 'xyz']
            vertices = np.empty((nv, 3), np.float64)
            for i in range(nv):
                words = f.readline().split()
                if len(words) < len(vprops):
                    raise bad('truncated body: vertex %d of %d' % (i, nv))
                try:
                    vertices[i] = [float(words[c]) for c in cols]
                except ValueError:
                    raise bad('vertex %d: not a number' % i)
            faces = np.empty((nf, 3), np.int64)
            for i in range(nf):
                words = f.readline().split()
                try:
                    if len(words) <= li:
                        raise bad('truncated body: face %d of %d' % (i, nf))
                    n = int(words[li])                          # scalars in front of the list hold one word each
                    if n != 3:
                        raise polygon(i, n)
                    if len(words) < len(fprops) + 3:
                        raise bad('truncated body: face %d of %d' % (i, nf))
                    faces[i] = [int(w) for w in words[li + 1:li + 4]]
                except ValueError as e:
                    raise e if str(e).startswith(path) else bad('face %d: not an integer' % i)
        else:
            order = '<' if fmt == 'binary_little_endian' else '>'
            vdtype = np.dtype([(n, order + t) for n, t, _ in vprops])
            body = f.read(nv * vdtype.itemsize)
            if len(body) != nv * vdtype.itemsize:
                raise bad('truncated body: %d bytes for %d vertices of %d bytes' % (len(body), nv, vdtype.itemsize))
            v = np.frombuffer(body, vdtype, nv)
            vertices = np.stack([v['x'], v['y'], v['z']], -1).reshape(nv, 3)
            fdtype = np.dtype([fld for p in fprops for fld in (
                [('_n', order + p[1]), ('_v', order + p[2], (3,))] if p[2] is not None else [('s_' + p[0], order + p[1])])])
            body = f.read(nf * fdtype.itemsize)                   # every face a triangle: records of one size
            t = np.frombuffer(body[:len(body) // fdtype.itemsize * fdtype.itemsize], fdtype)
            wrong = np.flatnonzero(t['_n'] != 3)
            if wrong.size:                                        # the first record that is no triangle is still aligned
                raise polygon(int(wrong[0]), int(t['_n'][wrong[0]]))
            if len(t) != nf:
                raise bad('truncated body: %d of %d faces' % (len(t), nf))
            faces = t['_v'].astype(np.int64).reshape(nf, 3)
    if nf and (faces.min() < 0 or faces.max() >= nv):
        raise bad('a face index outside 0..%d' % (nv - 1))
    return vertices.astype(np.float32).reshape(nv, 3), faces.astype(np.int32).reshape(nf, 3)
