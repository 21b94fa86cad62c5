"""A glTF 2.0 binary (.glb) writer for the rigged body (DESIGN.md sections 7n and 7o): struct, json and numpy only.

One mesh primitive (POSITION, optionally NORMAL, COLOR_0 as normalised bytes, JOINTS_n / WEIGHTS_n, uint32 indices), one skin of
the 24 SMPL joints, optionally one animation (a rotation and a translation channel per joint, LINEAR; a node above the root for
the world placement; one morph target per key with a STEP weights channel).  The file is in the body's own space: nothing is
rotated to glTF's +Y-up convention and nothing is rescaled.  The same inputs give the same bytes: no date, no host name, JSON
with sorted keys.  With texture= the primitive is unwelded (three vertices per triangle, TEXCOORD_0 into the per-triangle atlas of
DESIGN.md section 7o, no COLOR_0) and carries one PNG image, one sampler, one texture and one material; with joints=None the mesh
is static; with texture['normal_png'] / ['tangents'] it also carries TANGENT and a tangent-space normal map.
Several materials, cameras and several scenes are not written."""
import json
import struct

import numpy as np

from .synth import SMPL_PARENT

GENERATOR = 'occnerf_amd.gltf'
JOINT_NAMES = ('pelvis', 'left_hip', 'right_hip', 'spine1', 'left_knee', 'right_knee', 'spine2', 'left_ankle', 'right_ankle',
               'spine3', 'left_foot', 'right_foot', 'neck', 'left_collar', 'right_collar', 'head', 'left_shoulder',
               'right_shoulder', 'left_elbow', 'right_elbow', 'left_wrist', 'right_wrist', 'left_hand', 'right_hand')
N_JOINTS = len(JOINT_NAMES)
PARENTS = [-1] + [SMPL_PARENT[b] for b in range(1, N_JOINTS)]
FLOAT, UBYTE, UINT = 5126, 5121, 5125
ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 34962, 34963
LINEAR, CLAMP_TO_EDGE = 9729, 33071


def quaternion(R, previous=None):
    """The unit quaternion (x, y, z, w) float64 of the float64 3x3 matrix R by Shepperd's branch (the largest of the trace and
    the diagonal entries picks the component that is divided by), normalised; previous: the sign with the non-negative dot
    product against it, so that a linear interpolation takes the short way."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    pick = int(np.argmax([tr, R[0, 0], R[1, 1], R[2, 2]]))
    if pick == 0:
        w = 0.5 * np.sqrt(1.0 + tr)
        q = [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]
    else:
        i = pick - 1
        j, k = (i + 1) % 3, (i + 2) % 3
        a = 0.5 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / (4 * a)]
        q[i], q[j], q[k] = a, (R[j, i] + R[i, j]) / (4 * a), (R[k, i] + R[i, k]) / (4 * a)
    q = np.array(q, dtype=np.float64)
    q = q / np.sqrt((q * q).sum())
    if previous is not None and float((q * np.asarray(previous, dtype=np.float64)).sum()) < 0.0:
        q = -q
    return q


def rest_translations(cnl_gtfms):
    """[24,3] float64: every joint's rest offset from its parent (the root: from the origin), from the canonical global
    transforms [24,4,4]: the translation of inv(G_parent) G_b."""
    g = np.asarray(cnl_gtfms, dtype=np.float32).astype(np.float64).reshape(N_JOINTS, 4, 4)
    out = np.zeros((N_JOINTS, 3))
    for b in range(N_JOINTS):
        out[b] = g[b][:3, 3] if b == 0 else (np.linalg.inv(g[PARENTS[b]]) @ g[b])[:3, 3]
    return out


class _Buffer:
    def __init__(self):
        self.blob, self.views, self.accessors = bytearray(), [], []

    def add(self, array, ctype, kind, target=None, minmax=False, normalized=False):
        """One buffer view (aligned to 4 bytes) and one accessor over the array -> the accessor's index."""
        a = np.ascontiguousarray(array)
        self.blob.extend(b'\0' * (-len(self.blob) % 4))
        view = {'buffer': 0, 'byteOffset': len(self.blob), 'byteLength': a.nbytes}
        if target is not None:
            view['target'] = target
        self.blob.extend(a.tobytes())
        self.views.append(view)
        acc = {'bufferView': len(self.views) - 1, 'componentType': ctype, 'count': int(a.shape[0]), 'type': kind}
        if normalized:
            acc['normalized'] = True
        if minmax:
            flat = a.reshape(a.shape[0], -1).astype(np.float64)
            acc['min'], acc['max'] = flat.min(0).tolist(), flat.max(0).tolist()
        self.accessors.append(acc)
        return len(self.accessors) - 1


def write_glb(path, verts, faces, colors, joints, weights, cnl_gtfms, normals=None, animation=None, world=None, correctives=None,
              fps=30.0, texture=None):
    """The rigged mesh as <path> (glTF 2.0 binary) -> the number of bytes written.

    verts float32 [V,3], faces int32 [T,3], colors uint8 [V,3], normals float32 [V,3] or None; joints uint8 [V,K] and weights
    float32 [V,K] with K 4 or 8 (ops.mesh_skin's); cnl_gtfms [24,4,4]: the canonical global joint transforms (the rest pose;
    their inverses are the inverse bind matrices).  animation: None (the rest pose only) or {'rotation': [F,24,4] float64 unit
    quaternions (x, y, z, w), 'translation': [F,24,3]}: every joint's local transform per key (mesh.rig_frames), key i at
    i / fps seconds.  world: None or {'rotation': [F,4], 'translation': [F,3]}: a node above the root joint.  correctives:
    None or float32 [F,V,3]: one morph target per key, switched on at its key by a STEP weights channel.

    joints None (then weights and cnl_gtfms are not read): a static mesh -- no skin, no joint nodes, no animation.
    texture: None or {'uv': float32 [T,3,2] (mesh.texture_uv), 'png': the atlas as the bytes of a PNG file}: every per-vertex
    array is gathered by faces.reshape(-1), the indices are 0 .. 3T-1, TEXCOORD_0 replaces COLOR_0 (viewers multiply the two;
    colors may be None) and the image travels inside the binary chunk.  Without texture and with joints the bytes are those
    written before either was offered.  texture may also carry 'normal_png' (the tangent-space normal map of DESIGN.md section
    7q on the same atlas, a PNG file) and 'tangents' float32 [T,3,4] (mesh.corner_tangents; normals must be given): TANGENT is a
    float32 VEC4 per corner, a second image and texture share the sampler and materials[0].normalTexture names it; morph
    targets carry no tangent deltas.  Without the two keys the bytes are those written before they were offered."""
    verts = np.asarray(verts, dtype='<f4').reshape(-1, 3)
    faces = np.asarray(faces, dtype='<i4').reshape(-1, 3)
    V = verts.shape[0]
    rigged = joints is not None
    if texture is None or colors is not None:
        colors = np.asarray(colors, dtype=np.uint8).reshape(V, 3)
    K = 0
    if rigged:
        joints, weights = np.asarray(joints, dtype=np.uint8), np.asarray(weights, dtype='<f4')
        K = joints.shape[1] if joints.ndim == 2 else -1
        if K not in (4, 8) or joints.shape != (V, K) or weights.shape != (V, K):
            raise RuntimeError(f'write_glb: joints and weights must be [{V},K] with K 4 or 8, got {joints.shape} and {weights.shape}')
    elif animation is not None or world is not None or correctives is not None:
        raise RuntimeError('write_glb: a mesh without joints is static: it takes no animation, world placement or correctives')
    if V == 0 or faces.shape[0] == 0:
        raise RuntimeError('write_glb: a mesh without vertices or faces cannot be written (glTF accessors hold at least one element)')
    if (rigged and joints.max() >= N_JOINTS) or faces.min() < 0 or faces.max() >= V:
        raise RuntimeError(f'write_glb: a joint index reaches {N_JOINTS} or a face index lies outside [0, {V})')
    if texture is not None:
        uv, png = np.asarray(texture['uv'], dtype='<f4'), bytes(texture['png'])
        if uv.shape != (faces.shape[0], 3, 2) or png[:8] != b'\x89PNG\r\n\x1a\n':
            raise RuntimeError(f"write_glb: texture['uv'] must be float32 [{faces.shape[0]},3,2] and texture['png'] a PNG file, got "
                               f'{uv.shape} and {len(png)} bytes')
        if ('normal_png' in texture) != ('tangents' in texture):
            raise RuntimeError("write_glb: texture['normal_png'] and texture['tangents'] go together: a normal map needs its tangents")
        if 'normal_png' in texture:
            normal_png, tangents = bytes(texture['normal_png']), np.asarray(texture['tangents'], dtype='<f4')
            if tangents.shape != (faces.shape[0], 3, 4) or normal_png[:8] != b'\x89PNG\r\n\x1a\n':
                raise RuntimeError(f"write_glb: texture['tangents'] must be float32 [{faces.shape[0]},3,4] and texture['normal_png'] a "
                                   f'PNG file, got {tangents.shape} and {len(normal_png)} bytes')
            if normals is None:
                raise RuntimeError("write_glb: a normal map needs normals: glTF's TANGENT is read against NORMAL")
    fps = float(fps)
    if not (0.0 < fps < float('inf')):
        raise RuntimeError(f'write_glb: fps = {fps} must be a positive finite number')
    F = 0 if animation is None else int(np.asarray(animation['rotation']).shape[0])
    if correctives is not None and (animation is None or np.asarray(correctives).shape != (F, V, 3)):
        raise RuntimeError('write_glb: correctives are float32 [F,V,3] over the keys of an animation')
    if world is not None and animation is None:
        raise RuntimeError('write_glb: the world placement is animated: it needs an animation')

    buf = _Buffer()
    if normals is not None:
        normals = np.asarray(normals, dtype='<f4').reshape(V, 3)
    indices = faces.reshape(-1).astype('<u4')
    if texture is not None:                              # unwelded: a vertex per corner, in the order of the faces
        corner = faces.reshape(-1)
        verts, normals = verts[corner], None if normals is None else normals[corner]
        if rigged:
            joints, weights = joints[corner], weights[corner]
        if correctives is not None:
            correctives = np.asarray(correctives, dtype='<f4')[:, corner]
        indices = np.arange(corner.shape[0], dtype='<u4')
    attributes = {'POSITION': buf.add(verts, FLOAT, 'VEC3', ARRAY_BUFFER, minmax=True)}
    if normals is not None:
        attributes['NORMAL'] = buf.add(normals, FLOAT, 'VEC3', ARRAY_BUFFER)
    mapped = texture is not None and 'normal_png' in texture
    if mapped:                                           # per corner already: a row per vertex of the unwelded primitive
        attributes['TANGENT'] = buf.add(tangents.reshape(-1, 4), FLOAT, 'VEC4', ARRAY_BUFFER)
    if texture is None:
        rgba = np.concatenate([colors, np.full((V, 1), 255, np.uint8)], 1)
        attributes['COLOR_0'] = buf.add(rgba, UBYTE, 'VEC4', ARRAY_BUFFER, normalized=True)
    else:
        attributes['TEXCOORD_0'] = buf.add(uv.reshape(-1, 2), FLOAT, 'VEC2', ARRAY_BUFFER)
    for s in range(K // 4):
        attributes[f'JOINTS_{s}'] = buf.add(joints[:, 4 * s:4 * s + 4], UBYTE, 'VEC4', ARRAY_BUFFER)
        attributes[f'WEIGHTS_{s}'] = buf.add(weights[:, 4 * s:4 * s + 4], FLOAT, 'VEC4', ARRAY_BUFFER)
    primitive = {'attributes': attributes, 'indices': buf.add(indices, UINT, 'SCALAR', ELEMENT_ARRAY_BUFFER), 'mode': 4}
    mesh = {'primitives': [primitive], 'name': 'body'}
    image_view = None
    if texture is not None:                              # the PNG file as a buffer view of its own: no accessor, no target
        buf.blob.extend(b'\0' * (-len(buf.blob) % 4))
        buf.views.append({'buffer': 0, 'byteOffset': len(buf.blob), 'byteLength': len(png)})
        buf.blob.extend(png)
        image_view = len(buf.views) - 1
        primitive['material'] = 0
        if mapped:
            buf.blob.extend(b'\0' * (-len(buf.blob) % 4))
            buf.views.append({'buffer': 0, 'byteOffset': len(buf.blob), 'byteLength': len(normal_png)})
            buf.blob.extend(normal_png)
    if correctives is not None:
        d = np.asarray(correctives, dtype='<f4')
        primitive['targets'] = [{'POSITION': buf.add(d[f], FLOAT, 'VEC3', ARRAY_BUFFER, minmax=True)} for f in range(F)]
        mesh['weights'] = [0.0] * F

    if image_view is not None:
        extras = {'images': [{'bufferView': image_view, 'mimeType': 'image/png'}],
                  'samplers': [{'magFilter': LINEAR, 'minFilter': LINEAR, 'wrapS': CLAMP_TO_EDGE, 'wrapT': CLAMP_TO_EDGE}],
                  'textures': [{'sampler': 0, 'source': 0}],
                  'materials': [{'name': 'baked', 'pbrMetallicRoughness': {'baseColorTexture': {'index': 0}, 'metallicFactor': 0.0,
                                                                          'roughnessFactor': 1.0}}]}
        if mapped:                                       # a second image and texture on the one sampler
            extras['images'].append({'bufferView': image_view + 1, 'mimeType': 'image/png'})
            extras['textures'].append({'sampler': 0, 'source': 1})
            extras['materials'][0]['normalTexture'] = {'index': 1}
    else:
        extras = {}
    if not rigged:
        doc = {'asset': {'version': '2.0', 'generator': GENERATOR}, 'scene': 0, 'scenes': [{'nodes': [0]}],
               'nodes': [{'name': 'body', 'mesh': 0}], 'meshes': [mesh], **extras}
        return _finish(path, doc, buf)

    g = np.asarray(cnl_gtfms, dtype=np.float32).astype(np.float64).reshape(N_JOINTS, 4, 4)
    ibm = np.stack([np.linalg.inv(g[b]).T for b in range(N_JOINTS)]).astype('<f4')                  # column-major
    rest = rest_translations(g)
    first = 1                                            # node 0 carries the mesh; nodes 1 .. 24 are the joints
    nodes = [{'name': 'body', 'mesh': 0, 'skin': 0}]
    for b in range(N_JOINTS):
        node = {'name': JOINT_NAMES[b], 'translation': rest[b].tolist()}
        children = [first + c for c in range(N_JOINTS) if PARENTS[c] == b]
        if children:
            node['children'] = children
        nodes.append(node)
    top = first
    if world is not None:
        nodes.append({'name': 'world', 'children': [first]})
        top = len(nodes) - 1
    skin = {'joints': list(range(first, first + N_JOINTS)), 'skeleton': first, 'name': 'smpl',
            'inverseBindMatrices': buf.add(ibm.reshape(N_JOINTS, 16), FLOAT, 'MAT4')}
    doc = {'asset': {'version': '2.0', 'generator': GENERATOR}, 'scene': 0, 'scenes': [{'nodes': [0, top]}], 'nodes': nodes,
           'meshes': [mesh], 'skins': [skin], **extras}

    if animation is not None:
        rot = np.asarray(animation['rotation'], dtype=np.float64).reshape(F, N_JOINTS, 4)
        tra = np.asarray(animation['translation'], dtype=np.float64).reshape(F, N_JOINTS, 3)
        t_in = buf.add((np.arange(F, dtype=np.float64) / fps).astype('<f4'), FLOAT, 'SCALAR', minmax=True)
        samplers, channels = [], []

        def channel(node, prop, values, kind, interpolation='LINEAR'):
            samplers.append({'input': t_in, 'output': buf.add(values.astype('<f4'), FLOAT, kind), 'interpolation': interpolation})
            channels.append({'sampler': len(samplers) - 1, 'target': {'node': node, 'path': prop}})
        for b in range(N_JOINTS):
            channel(first + b, 'rotation', rot[:, b], 'VEC4')
            channel(first + b, 'translation', tra[:, b], 'VEC3')
        if world is not None:
            channel(top, 'rotation', np.asarray(world['rotation'], dtype=np.float64).reshape(F, 4), 'VEC4')
            channel(top, 'translation', np.asarray(world['translation'], dtype=np.float64).reshape(F, 3), 'VEC3')
        if correctives is not None:
            channel(0, 'weights', np.eye(F).reshape(F * F), 'SCALAR', 'STEP')
        doc['animations'] = [{'name': 'capture', 'samplers': samplers, 'channels': channels}]
    return _finish(path, doc, buf)


def _finish(path, doc, buf):
    """The document and its buffer as the two chunks of <path> -> the number of bytes written."""
    buf.blob.extend(b'\0' * (-len(buf.blob) % 4))
    doc['buffers'] = [{'byteLength': len(buf.blob)}]
    doc['bufferViews'], doc['accessors'] = buf.views, buf.accessors
    text = json.dumps(doc, sort_keys=True, separators=(',', ':')).encode('utf-8')
    text += b' ' * (-len(text) % 4)
    total = 12 + 8 + len(text) + 8 + len(buf.blob)
    with open(path, 'wb') as out:
        out.write(struct.pack('<4sII', b'glTF', 2, total))
        out.write(struct.pack('<I4s', len(text), b'JSON'))
        out.write(text)
        out.write(struct.pack('<I4s', len(buf.blob), b'BIN\0'))
        out.write(bytes(buf.blob))
    return total
