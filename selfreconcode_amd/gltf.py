"""Binary glTF 2.0 for the skinned avatar, on the standard library and numpy: the writer, this package's own reader,
a validator of the specification's structural rules, and a replay -- the specification's morphing and vertex skinning written out
from a file's contents alone, in float64 -- that stands in for a viewer.

The file holds one mesh primitive (POSITION, NORMAL, TEXCOORD_0, JOINTS_n / WEIGHTS_n, morph targets, indices), a skin of 24 joints
whose hierarchy and rest offsets are the skinner's and whose inverse bind matrices are its `init_pose`, the root joint under a node that
carries the translation, an optional material with the texture's PNG bytes embedded, and one animation: a rotation channel per
joint, the translation channel and a `weights` channel for the morph coefficients, keyed at k / fps.  Coordinates are the model's own
(SMPL's, y-up); no camera is written.

Texture coordinates: the package's atlas puts texel row r, column c at (u, v) = ((c + 0.5) / R, 1 - (r + 0.5) / R) (csrc/texture.hip:
v grows upwards, row 0 is the top of texture.png); glTF's origin is the image's top-left corner with v growing downwards, so the file
stores (u, 1 - v) (`gltf_uv`)."""
import json
import struct

import numpy as np

MAGIC, VERSION = 0x46546C67, 2
CHUNK_JSON, CHUNK_BIN = 0x4E4F534A, 0x004E4942
BYTE, UBYTE, SHORT, USHORT, UINT, FLOAT = 5120, 5121, 5122, 5123, 5125, 5126
COMPONENTS = {BYTE: np.dtype('i1'), UBYTE: np.dtype('u1'), SHORT: np.dtype('<i2'), USHORT: np.dtype('<u2'), UINT: np.dtype('<u4'), FLOAT: np.dtype('<f4')}
TYPES = {'SCALAR': 1, 'VEC2': 2, 'VEC3': 3, 'VEC4': 4, 'MAT2': 4, 'MAT3': 9, 'MAT4': 16}
ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 34962, 34963
WEIGHT_SUM_TOL = 1e-6           # |sum of a vertex's weights - 1| a file may show: float32 weights that sum to 1 within 2 ulp pass
UNIT_TOL = 1e-5                 # |q| - 1 of a stored rotation
REPLAY_FRAMES = 8               # frames the replay skins at once


class GltfError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------- seams and texture coordinates
def gltf_uv(vt):
    """The package's texture coordinates vt [...,2] (v upwards) as glTF's (v downwards): (u, 1 - v), float32."""
    vt = np.asarray(vt, np.float32)
    return np.stack([vt[..., 0], np.float32(1.) - vt[..., 1]], -1)


def texel_of(uv, R):
    """(row, column) of the texel of an R x R image that glTF's texture coordinate uv [...,2] falls in: the origin is the image's
    top-left corner, u along a row, v down the rows."""
    uv = np.asarray(uv, np.float64)
    cell = np.clip(np.floor(uv * R), 0, R - 1).astype(np.int64)
    return cell[..., 1], cell[..., 0]


def split_seams(faces, ft, vt):
    """A mesh whose faces index vertices (`faces` [F,3]) and texture coordinates (`ft` [F,3] into vt [Vt,2]) apart, as one index per
    corner: the unique (vertex, uv bits) pairs -> (origin [V'] the vertex each new vertex copies, uv [V',2] float32 as stored in vt,
    new_faces [F,3])."""
    faces, ft = np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(ft, np.int64).reshape(-1, 3)
    vt = np.ascontiguousarray(vt, np.float32).reshape(-1, 2)
    if faces.shape != ft.shape:
        raise ValueError(f"split_seams: faces {faces.shape} and ft {ft.shape} must correspond one to one")
    bits = vt.view(np.uint32).astype(np.int64)[ft.reshape(-1)]
    keys = np.concatenate([faces.reshape(-1, 1), bits], 1)
    unique, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    return unique[:, 0].copy(), vt[ft.reshape(-1)[first]], inverse.reshape(-1, 3).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- the writer
class _Buffer:
    def __init__(self):
        self.data, self.views, self.accessors = bytearray(), [], []

    def view(self, raw, target=None):
        self.data += b"\0" * (-len(self.data) % 4)
        view = {'buffer': 0, 'byteOffset': len(self.data), 'byteLength': len(raw)}
        if target is not None:
            view['target'] = target
        self.data += raw
        self.views.append(view)
        return len(self.views) - 1

    def accessor(self, array, component, kind, target=None, bounds=False):
        array = np.ascontiguousarray(array, COMPONENTS[component]).reshape(-1, TYPES[kind])
        acc = {'bufferView': self.view(array.tobytes(), target), 'componentType': component, 'count': int(array.shape[0]), 'type': kind}
        if bounds:
            acc['min'], acc['max'] = [float(x) for x in array.min(0)], [float(x) for x in array.max(0)]
        self.accessors.append(acc)
        return len(self.accessors) - 1


def pack_glb(document, binary):
    """The bytes of a .glb from its JSON document and its binary chunk."""
    text = json.dumps(document, separators=(',', ':'), allow_nan=False).encode('utf-8')
    text += b" " * (-len(text) % 4)
    binary = bytes(binary) + b"\0" * (-len(binary) % 4)
    total = 12 + 8 + len(text) + 8 + len(binary)
    return (struct.pack('<III', MAGIC, VERSION, total) + struct.pack('<II', len(text), CHUNK_JSON) + text
            + struct.pack('<II', len(binary), CHUNK_BIN) + binary)


def _sets(joints, weights):
    """joints / weights [V,K] as K' = 4 or 8 columns: JOINTS_0 / WEIGHTS_0 and, past four influences, _1."""
    V, K = joints.shape
    width = 4 if K <= 4 else 8
    j, w = np.zeros((V, width), np.uint8), np.zeros((V, width), np.float32)
    j[:, :K], w[:, :K] = joints, weights
    return [(j[:, s:s + 4], w[:, s:s + 4]) for s in range(0, width, 4)]


def write_glb(path, positions, faces, joints, weights, parents, joint_positions, inverse_bind, quaternions, translations, fps=30.,
              normals=None, uvs=None, morphs=None, morph_weights=None, texture_png=None, generator="selfreconcode_amd.gltf"):
    """Writes the avatar as binary glTF 2.0.
    positions [V,3] the rest mesh; faces [F,3]; joints [V,K] (0 <= joint < J) / weights [V,K] (K in 1..8, rows summing to 1; unused
    slots joint 0, weight 0); parents [J] (-1, or anything negative, for the one root), joint_positions [J,3] the rest joints,
    inverse_bind [J,4,4] (row major here, stored column major); quaternions [T,J,4] as (w, x, y, z) -- normalised and stored as glTF's
    (x, y, z, w) float32 --, translations [T,3] of the node above the root joint, key times k / fps.  Optional: normals [V,3], uvs
    [V,2] already in glTF's orientation (gltf_uv), morphs [B,V,3] displacement targets with morph_weights [T,B], texture_png the
    bytes of a PNG for the base colour.  Returns the document (the JSON chunk as a dict)."""
    positions = np.asarray(positions, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    joints, weights = np.asarray(joints), np.asarray(weights, np.float32)
    V, J = positions.shape[0], len(parents)
    quaternions = np.asarray(quaternions, np.float64)
    translations = np.asarray(translations, np.float64).reshape(-1, 3)
    T = quaternions.shape[0]
    if joints.ndim != 2 or joints.shape != weights.shape or joints.shape[0] != V or not 1 <= joints.shape[1] <= 8:
        raise ValueError(f"write_glb: joints / weights [{V},K] with K in 1..8 expected, got {joints.shape} and {weights.shape}")
    if joints.min() < 0 or joints.max() >= J or J > 255:
        raise ValueError(f"write_glb: joints in [0, {J}) expected (at most 255 joints)")
    if faces.size and (faces.min() < 0 or faces.max() >= V):
        raise ValueError(f"write_glb: faces index [{faces.min()}, {faces.max()}], past the {V} vertices")
    if quaternions.shape != (T, J, 4) or translations.shape != (T, 3) or T == 0 or not float(fps) > 0.:
        raise ValueError(f"write_glb: quaternions [T,{J},4], translations [T,3] with T > 0 and fps > 0 expected")
    roots = [i for i, p in enumerate(parents) if int(p) < 0 or i == 0]
    if roots != [0]:
        raise ValueError("write_glb: joint 0 is the one root expected")
    B = 0 if morphs is None else int(np.asarray(morphs).shape[0])
    if B:
        morphs, morph_weights = np.asarray(morphs, np.float32).reshape(B, -1, 3), np.asarray(morph_weights, np.float32)
        if morphs.shape[1] != V or morph_weights.shape != (T, B):
            raise ValueError(f"write_glb: morphs [B,{V},3] and morph_weights [{T},B] expected")
    buf = _Buffer()
    attributes = {'POSITION': buf.accessor(positions, FLOAT, 'VEC3', ARRAY_BUFFER, bounds=True)}
    if normals is not None:
        attributes['NORMAL'] = buf.accessor(np.asarray(normals, np.float32).reshape(V, 3), FLOAT, 'VEC3', ARRAY_BUFFER)
    if uvs is not None:
        attributes['TEXCOORD_0'] = buf.accessor(np.asarray(uvs, np.float32).reshape(V, 2), FLOAT, 'VEC2', ARRAY_BUFFER)
    for s, (j4, w4) in enumerate(_sets(joints, weights)):
        attributes['JOINTS_%d' % s] = buf.accessor(j4, UBYTE, 'VEC4', ARRAY_BUFFER)
        attributes['WEIGHTS_%d' % s] = buf.accessor(w4, FLOAT, 'VEC4', ARRAY_BUFFER)
    primitive = {'attributes': attributes, 'indices': buf.accessor(faces.reshape(-1), UINT, 'SCALAR', ELEMENT_ARRAY_BUFFER), 'mode': 4}
    mesh = {'primitives': [primitive], 'name': 'avatar'}
    if B:
        primitive['targets'] = [{'POSITION': buf.accessor(morphs[b], FLOAT, 'VEC3', ARRAY_BUFFER, bounds=True)} for b in range(B)]
        mesh['weights'] = [0.] * B
    Js = np.asarray(joint_positions, np.float64).reshape(J, 3)
    nodes = []
    for i in range(J):
        local = Js[i] - (Js[int(parents[i])] if i else 0.)
        node = {'name': 'joint_%d' % i, 'translation': [float(x) for x in local], 'rotation': [0., 0., 0., 1.]}
        children = [c for c in range(1, J) if int(parents[c]) == i]
        if children:
            node['children'] = children
        nodes.append(node)
    motion_node, mesh_node = J, J + 1
    nodes.append({'name': 'motion', 'children': [0], 'translation': [0., 0., 0.]})
    nodes.append({'name': 'avatar', 'mesh': 0, 'skin': 0})
    ibm = np.asarray(inverse_bind, np.float32).reshape(J, 4, 4).transpose(0, 2, 1)                 # column major
    skin = {'joints': list(range(J)), 'skeleton': 0, 'inverseBindMatrices': buf.accessor(ibm.reshape(J, 16), FLOAT, 'MAT4')}
    document = {'asset': {'version': '2.0', 'generator': generator}, 'scene': 0, 'scenes': [{'nodes': [motion_node, mesh_node]}], 'nodes': nodes,
                'meshes': [mesh], 'skins': [skin]}
    if texture_png is not None:
        document['images'] = [{'bufferView': buf.view(bytes(texture_png)), 'mimeType': 'image/png'}]
        document['samplers'] = [{'magFilter': 9729, 'minFilter': 9987, 'wrapS': 33071, 'wrapT': 33071}]
        document['textures'] = [{'source': 0, 'sampler': 0}]
        document['materials'] = [{'name': 'avatar', 'pbrMetallicRoughness': {'baseColorTexture': {'index': 0}, 'metallicFactor': 0., 'roughnessFactor': 1.}}]
    else:
        document['materials'] = [{'name': 'avatar', 'pbrMetallicRoughness': {'baseColorFactor': [0.8, 0.8, 0.8, 1.], 'metallicFactor': 0., 'roughnessFactor': 1.}}]
    primitive['material'] = 0
    times = buf.accessor(np.arange(T, dtype=np.float64) / float(fps), FLOAT, 'SCALAR', bounds=True)
    unit = quaternions / np.linalg.norm(quaternions, axis=-1, keepdims=True)
    samplers, channels = [], []

    def channel(node, path, output):
        samplers.append({'input': times, 'output': output, 'interpolation': 'LINEAR'})
        channels.append({'sampler': len(samplers) - 1, 'target': {'node': node, 'path': path}})
    for i in range(J):
        channel(i, 'rotation', buf.accessor(unit[:, i][:, [1, 2, 3, 0]], FLOAT, 'VEC4'))
    channel(motion_node, 'translation', buf.accessor(translations, FLOAT, 'VEC3'))
    if B:
        channel(mesh_node, 'weights', buf.accessor(morph_weights.reshape(-1), FLOAT, 'SCALAR'))
    document['animations'] = [{'name': 'clip', 'samplers': samplers, 'channels': channels}]
    document['accessors'], document['bufferViews'] = buf.accessors, buf.views
    binary = bytes(buf.data) + b"\0" * (-len(buf.data) % 4)
    document['buffers'] = [{'byteLength': len(binary)}]
    with open(path, 'wb') as fh:
        fh.write(pack_glb(document, binary))
    return document


# ---------------------------------------------------------------------------------------------------- the reader
def _fail(message):
    raise GltfError("glb: " + message)


def split_glb(blob):
    """(document, binary) of a .glb's bytes: header, JSON chunk, BIN chunk; GltfError for a broken container."""
    if len(blob) < 20:
        _fail("shorter than a header and a chunk header")
    magic, version, total = struct.unpack_from('<III', blob, 0)
    if magic != MAGIC:
        _fail("the magic is not 'glTF'")
    if version != VERSION:
        _fail(f"version {version}, 2 expected")
    if total != len(blob):
        _fail(f"the header says {total} bytes, the file has {len(blob)}")
    if total % 4:
        _fail("the length is no multiple of 4")
    at, chunks = 12, []
    while at < total:
        if at + 8 > total:
            _fail("a chunk header runs past the end")
        length, kind = struct.unpack_from('<II', blob, at)
        if length % 4:
            _fail(f"a chunk of {length} bytes: no multiple of 4")
        if at + 8 + length > total:
            _fail("a chunk runs past the end")
        chunks.append((kind, blob[at + 8:at + 8 + length]))
        at += 8 + length
    if not chunks or chunks[0][0] != CHUNK_JSON:
        _fail("the first chunk is not JSON")
    if len(chunks) > 1 and chunks[1][0] != CHUNK_BIN:
        _fail("the second chunk is not BIN")
    try:
        document = json.loads(bytes(chunks[0][1]).decode('utf-8'))
    except (UnicodeDecodeError, ValueError) as e:
        _fail(f"the JSON chunk does not parse: {e}")
    return document, bytes(chunks[1][1]) if len(chunks) > 1 else b""


def _accessor_array(document, binary, index):
    """Accessor `index` as an array [count, components] (a copy), every rule on the way checked."""
    accessors, views = document.get('accessors', []), document.get('bufferViews', [])
    if not isinstance(index, int) or not 0 <= index < len(accessors):
        _fail(f"accessor {index} does not exist")
    acc = accessors[index]
    component, kind, count = acc.get('componentType'), acc.get('type'), acc.get('count')
    if component not in COMPONENTS:
        _fail(f"accessor {index}: component type {component}")
    if kind not in TYPES:
        _fail(f"accessor {index}: type {kind!r}")
    if not isinstance(count, int) or count < 1:
        _fail(f"accessor {index}: count {count}")
    if 'sparse' in acc or 'bufferView' not in acc:
        _fail(f"accessor {index}: sparse or without a buffer view (not read here)")
    if not 0 <= acc['bufferView'] < len(views):
        _fail(f"accessor {index}: buffer view {acc['bufferView']} does not exist")
    view = views[acc['bufferView']]
    dtype, width = COMPONENTS[component], TYPES[kind]
    item = dtype.itemsize * width
    stride = view.get('byteStride', item)
    start = view.get('byteOffset', 0) + acc.get('byteOffset', 0)
    if start % dtype.itemsize or stride % dtype.itemsize:
        _fail(f"accessor {index}: offset {start} or stride {stride} is no multiple of the component size {dtype.itemsize}")
    if stride < item:
        _fail(f"accessor {index}: stride {stride} below the element size {item}")
    if acc.get('byteOffset', 0) + stride * (count - 1) + item > view['byteLength']:
        _fail(f"accessor {index} runs past its buffer view")
    rows = np.lib.stride_tricks.as_strided(np.frombuffer(binary, np.uint8, offset=start, count=stride * (count - 1) + item), (count, item), (stride, 1))
    return np.ascontiguousarray(rows).view(dtype).reshape(count, width).copy()


def read_glb(path):
    """{'json': the document, 'bin': the binary chunk, 'accessors': [array [count, components] per accessor]} of a .glb file (or its
    bytes).  GltfError for a broken container, view or accessor."""
    if isinstance(path, (bytes, bytearray)):
        blob = bytes(path)
    else:
        with open(path, 'rb') as fh:
            blob = fh.read()
    document, binary = split_glb(blob)
    _check_views(document, binary)
    return {'json': document, 'bin': binary, 'accessors': [_accessor_array(document, binary, i) for i in range(len(document.get('accessors', [])))]}


def _check_views(document, binary):
    buffers = document.get('buffers', [])
    if len(buffers) > 1 or (buffers and 'uri' in buffers[0]):
        _fail("one buffer, the BIN chunk, expected")
    if buffers and not buffers[0].get('byteLength', 0) <= len(binary):
        _fail(f"the buffer's {buffers[0].get('byteLength')} bytes exceed the BIN chunk's {len(binary)}")
    if buffers and len(binary) - buffers[0]['byteLength'] > 3:
        _fail("the BIN chunk is more than padding longer than the buffer")
    size = buffers[0]['byteLength'] if buffers else 0
    for i, view in enumerate(document.get('bufferViews', [])):
        offset, length = view.get('byteOffset', 0), view.get('byteLength')
        if view.get('buffer') != 0 or not isinstance(length, int) or length < 1 or not isinstance(offset, int) or offset < 0:
            _fail(f"buffer view {i}: buffer, offset or length")
        if offset + length > size:
            _fail(f"buffer view {i} runs past the buffer")
        if view.get('target') in (ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER) and offset % 4:
            _fail(f"buffer view {i}: vertex data at offset {offset}, no multiple of 4")


# ---------------------------------------------------------------------------------------------------- the validator
def _primitive(glb):
    meshes = glb['json'].get('meshes', [])
    if len(meshes) != 1 or len(meshes[0].get('primitives', [])) != 1:
        _fail("one mesh with one primitive expected")
    return meshes[0], meshes[0]['primitives'][0]


def _influences(glb, attributes):
    sets = 0
    while 'JOINTS_%d' % sets in attributes:
        sets += 1
    if sets == 0 or any(('WEIGHTS_%d' % s) not in attributes for s in range(sets)) or ('WEIGHTS_%d' % sets) in attributes:
        _fail("JOINTS_n and WEIGHTS_n do not pair up")
    joints = np.concatenate([glb['accessors'][attributes['JOINTS_%d' % s]] for s in range(sets)], 1)
    weights = np.concatenate([glb['accessors'][attributes['WEIGHTS_%d' % s]] for s in range(sets)], 1)
    return joints, weights


def validate_glb(path):
    """Checks the structural rules of the specification that this package's files must meet and returns read_glb's dict: magic, version
    and lengths; 4-byte alignment of chunks and vertex data, component alignment of accessors; buffer-view and accessor bounds;
    component and type codes; POSITION's min / max (present and true, the morph targets' too); vertex counts equal over the
    attributes; indices in range; the inverseBindMatrices count; joints in range; weights >= 0 summing to 1; unit rotations; strictly
    increasing sampler inputs with true min / max; output counts, a `weights` output of T B values.  GltfError names the first rule
    broken."""
    glb = read_glb(path)
    doc, acc = glb['json'], glb['accessors']
    if doc.get('asset', {}).get('version') != '2.0':
        _fail("asset.version is not '2.0'")
    mesh, prim = _primitive(glb)
    attributes = prim.get('attributes', {})
    if 'POSITION' not in attributes:
        _fail("no POSITION")
    count = None
    spec = {'POSITION': (FLOAT, 'VEC3'), 'NORMAL': (FLOAT, 'VEC3'), 'TEXCOORD_0': (FLOAT, 'VEC2')}
    for name, index in attributes.items():
        a = doc['accessors'][index]
        want = spec.get(name) or ((None, 'VEC4') if name.startswith(('JOINTS_', 'WEIGHTS_')) else None)
        if want is None:
            _fail(f"attribute {name} is not one this package writes")
        if a['type'] != want[1] or (want[0] is not None and a['componentType'] != want[0]):
            _fail(f"attribute {name}: component type {a['componentType']}, type {a['type']}")
        if name.startswith('JOINTS_') and a['componentType'] not in (UBYTE, USHORT):
            _fail(f"attribute {name}: component type {a['componentType']}")
        if name.startswith('WEIGHTS_') and a['componentType'] != FLOAT:
            _fail(f"attribute {name}: component type {a['componentType']} (float weights expected)")
        if count is not None and a['count'] != count:
            _fail(f"attribute {name}: {a['count']} elements, {count} expected")
        count = a['count']
        if not np.isfinite(acc[index].astype(np.float64)).all():
            _fail(f"attribute {name}: non-finite values")
    targets = prim.get('targets', [])
    for index in [attributes['POSITION']] + [t.get('POSITION') for t in targets]:
        if index is None:
            _fail("a morph target without POSITION")
        a = doc['accessors'][index]
        if a['count'] != count or a['type'] != 'VEC3' or a['componentType'] != FLOAT:
            _fail(f"accessor {index}: a position accessor of another count or type")
        if 'min' not in a or 'max' not in a:
            _fail(f"accessor {index}: POSITION without min / max")
        if not (np.array_equal(np.asarray(a['min'], np.float32), acc[index].min(0)) and np.array_equal(np.asarray(a['max'], np.float32), acc[index].max(0))):
            _fail(f"accessor {index}: POSITION min / max are not the data's")
    if 'indices' in prim:
        a = doc['accessors'][prim['indices']]
        if a['type'] != 'SCALAR' or a['componentType'] not in (UBYTE, USHORT, UINT) or a['count'] % 3:
            _fail("indices: unsigned scalars in threes expected")
        if int(acc[prim['indices']].max()) >= count:
            _fail("an index past the vertices")
    skins = doc.get('skins', [])
    if len(skins) != 1:
        _fail("one skin expected")
    skin_joints = skins[0].get('joints', [])
    nodes = doc.get('nodes', [])
    if not skin_joints or any(not isinstance(j, int) or not 0 <= j < len(nodes) for j in skin_joints) or len(set(skin_joints)) != len(skin_joints):
        _fail("skin.joints: distinct nodes expected")
    if 'inverseBindMatrices' in skins[0]:
        a = doc['accessors'][skins[0]['inverseBindMatrices']]
        if a['type'] != 'MAT4' or a['componentType'] != FLOAT:
            _fail("inverseBindMatrices: float MAT4 expected")
        if a['count'] != len(skin_joints):
            _fail(f"inverseBindMatrices: {a['count']} matrices for {len(skin_joints)} joints")
    parent = {}
    for i, node in enumerate(nodes):
        for c in node.get('children', []):
            if not isinstance(c, int) or not 0 <= c < len(nodes) or c in parent:
                _fail(f"node {c}: no node, or a second parent")
            parent[c] = i
    joints, weights = _influences(glb, attributes)
    if int(joints.max()) >= len(skin_joints):
        _fail(f"joint index {int(joints.max())} with {len(skin_joints)} joints")
    if (weights < 0.).any():
        _fail("a negative weight")
    off = np.abs(weights.astype(np.float64).sum(1) - 1.)
    if (off > WEIGHT_SUM_TOL).any():
        _fail(f"weights of vertex {int(off.argmax())} sum to 1 {'+' if weights[off.argmax()].astype(np.float64).sum() > 1 else '-'} {off.max():.3g}")
    if ((weights == 0.) & (joints != 0)).any():
        _fail("an unused influence with a joint other than 0")
    B = len(targets)
    if B and len(mesh.get('weights', [])) != B:
        _fail("mesh.weights does not match the morph targets")
    for n, anim in enumerate(doc.get('animations', [])):
        samplers = anim.get('samplers', [])
        for ch in anim.get('channels', []):
            if not isinstance(ch.get('sampler'), int) or not 0 <= ch['sampler'] < len(samplers):
                _fail(f"animation {n}: a channel without its sampler")
            s, target = samplers[ch['sampler']], ch.get('target', {})
            a_in, a_out = doc['accessors'][s['input']], doc['accessors'][s['output']]
            times = acc[s['input']][:, 0]
            if a_in['type'] != 'SCALAR' or a_in['componentType'] != FLOAT:
                _fail(f"animation {n}: a sampler input that is not float scalars")
            if 'min' not in a_in or 'max' not in a_in or np.float32(a_in['min'][0]) != times.min() or np.float32(a_in['max'][0]) != times.max():
                _fail(f"animation {n}: a sampler input without true min / max")
            if times[0] < 0. or (np.diff(times) <= 0.).any():
                _fail(f"animation {n}: sampler input times do not increase strictly")
            path, node = target.get('path'), target.get('node')
            if not isinstance(node, int) or not 0 <= node < len(nodes):
                _fail(f"animation {n}: a channel's node does not exist")
            T = times.shape[0]
            if path == 'rotation':
                if a_out['type'] != 'VEC4' or a_out['count'] != T:
                    _fail(f"animation {n}: rotation output of {a_out['count']} {a_out['type']} for {T} keys")
                if (np.abs(np.linalg.norm(acc[s['output']].astype(np.float64), axis=1) - 1.) > UNIT_TOL).any():
                    _fail(f"animation {n}: a rotation that is no unit quaternion")
            elif path in ('translation', 'scale'):
                if a_out['type'] != 'VEC3' or a_out['count'] != T:
                    _fail(f"animation {n}: {path} output of {a_out['count']} {a_out['type']} for {T} keys")
            elif path == 'weights':
                if 'mesh' not in nodes[node] or a_out['type'] != 'SCALAR' or a_out['count'] != T * B:
                    _fail(f"animation {n}: weights output of {a_out['count']} values for {T} keys of {B} targets")
            else:
                _fail(f"animation {n}: path {path!r}")
    for image in doc.get('images', []):
        if 'bufferView' in image and image.get('mimeType') not in ('image/png', 'image/jpeg'):
            _fail("an embedded image without its mimeType")
    return glb


# ---------------------------------------------------------------------------------------------------- the replay
def _rotation(q):
    """[...,4] (x, y, z, w) -> [...,3,3], the specification's matrix of a unit quaternion."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def replay_glb(glb, morphs=True, joints_weights=None):
    """The animation of a file played by the specification's rules, from the file's contents alone (read_glb's dict, or a path) ->
    [T,V,3] float64, frame k at the k-th key time: node TRS from the samplers' outputs (a node without a channel keeps its own),
    global transforms down the hierarchy, morphed positions POSITION + sum_b w_b target_b, joint matrices inverse(mesh node's global)
    global(joint) inverseBind, and sum_k weight_k (joint matrix_k [p; 1]).  morphs=False plays the skin alone; joints_weights =
    (joints [V,K], weights [V,K]) plays other influences than the file's."""
    if not isinstance(glb, dict):
        glb = read_glb(glb)
    doc, acc = glb['json'], [a.astype(np.float64) if a.dtype.kind == 'f' else a for a in glb['accessors']]
    mesh, prim = _primitive(glb)
    nodes = doc['nodes']
    mesh_node = [i for i, n in enumerate(nodes) if 'mesh' in n][0]
    skin = doc['skins'][nodes[mesh_node]['skin']]
    anim = doc['animations'][0]
    keyed = {}
    T = None
    for ch in anim['channels']:
        s = anim['samplers'][ch['sampler']]
        keyed[(ch['target']['node'], ch['target']['path'])] = acc[s['output']]
        T = acc[s['input']].shape[0] if T is None else T
        if acc[s['input']].shape[0] != T:
            _fail("replay: samplers of different key counts")
    N = len(nodes)
    local = np.zeros((T, N, 4, 4))
    for i, node in enumerate(nodes):
        if 'matrix' in node:
            local[:, i] = np.asarray(node['matrix'], np.float64).reshape(4, 4).T
            continue
        rot = keyed.get((i, 'rotation'), np.broadcast_to(np.asarray(node.get('rotation', [0., 0., 0., 1.]), np.float64), (T, 4)))
        tr = keyed.get((i, 'translation'), np.broadcast_to(np.asarray(node.get('translation', [0., 0., 0.]), np.float64), (T, 3)))
        sc = keyed.get((i, 'scale'), np.broadcast_to(np.asarray(node.get('scale', [1., 1., 1.]), np.float64), (T, 3)))
        local[:, i, :3, :3] = _rotation(rot / np.linalg.norm(rot, axis=-1, keepdims=True)) * sc[:, None, :]
        local[:, i, :3, 3] = tr
        local[:, i, 3, 3] = 1.
    parent = {c: i for i, node in enumerate(nodes) for c in node.get('children', [])}
    world = [None] * N

    def global_of(i):
        if world[i] is None:
            world[i] = local[:, i] if i not in parent else global_of(parent[i]) @ local[:, i]
        return world[i]
    J = len(skin['joints'])
    ibm = acc[skin['inverseBindMatrices']].reshape(J, 4, 4).transpose(0, 2, 1) if 'inverseBindMatrices' in skin else np.broadcast_to(np.eye(4), (J, 4, 4))
    inv_mesh = np.linalg.inv(global_of(mesh_node))
    joint_matrix = np.stack([inv_mesh @ global_of(j) @ ibm[n] for n, j in enumerate(skin['joints'])], 1)          # [T,J,4,4]
    p = np.broadcast_to(acc[prim['attributes']['POSITION']], (T,) + acc[prim['attributes']['POSITION']].shape).copy()
    targets = prim.get('targets', [])
    if morphs and targets:
        w = keyed.get((mesh_node, 'weights'))
        w = np.broadcast_to(np.asarray(mesh.get('weights', [0.] * len(targets)), np.float64), (T, len(targets))) if w is None else w.reshape(T, len(targets))
        for b, target in enumerate(targets):
            p += w[:, b, None, None] * acc[target['POSITION']][None]
    joints, weights = _influences(glb, prim['attributes']) if joints_weights is None else joints_weights
    joints, weights = np.asarray(joints, np.int64), np.asarray(weights, np.float64)
    out = np.zeros_like(p)
    for t0 in range(0, T, REPLAY_FRAMES):
        sl = slice(t0, t0 + REPLAY_FRAMES)
        for k in range(joints.shape[1]):
            Mk = joint_matrix[sl][:, joints[:, k]]                                                              # [t,V,4,4]
            out[sl] += weights[None, :, k, None] * (np.einsum('tvxc,tvc->tvx', Mk[..., :3, :3], p[sl]) + Mk[..., :3, 3])
    return out
