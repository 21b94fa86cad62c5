"""A minimal reader of glTF 2.0 binaries and a float64 evaluator of the glTF 2.0 equations, for the files of occnerf_amd/gltf.py
(DESIGN.md section 7n).  Nothing here is shared with the writer.

  parse       the 12-byte header and the JSON and BIN chunks -> (document, buffer);
  accessor    an accessor's elements as a numpy array [count, components] (tightly packed views only: the writer's);
  check_rules the structural rules of the specification the writer has to keep, as assertions;
  evaluate    the vertex positions at a time t: node hierarchy, LINEAR (slerp for rotations) and STEP sampling, morph targets
              before the skin, jointMatrix = inv(meshGlobal) jointGlobal inverseBindMatrix, the skinned vertex in world space
              = meshGlobal (sum_k w_k jointMatrix_k) p;
  chain_bound / corrective_bound: how far that evaluation may be from the definition's numbers, derived below."""
import json
import struct

import numpy as np

COMPONENTS = {'SCALAR': 1, 'VEC2': 2, 'VEC3': 3, 'VEC4': 4, 'MAT4': 16}
DTYPES = {5120: 'i1', 5121: 'u1', 5122: '<i2', 5123: '<u2', 5125: '<u4', 5126: '<f4'}
LONGEST_CHAIN = 9            # joints on the longest SMPL chain: pelvis, spine1-3, collar, shoulder, elbow, wrist, hand


def parse(blob):
    magic, version, length = struct.unpack_from('<4sII', blob, 0)
    assert magic == b'glTF' and version == 2 and length == len(blob), (magic, version, length, len(blob))
    n_json, kind = struct.unpack_from('<I4s', blob, 12)
    assert kind == b'JSON' and n_json % 4 == 0
    text = blob[20:20 + n_json]
    n_bin, kind = struct.unpack_from('<I4s', blob, 20 + n_json)
    assert kind == b'BIN\0' and n_bin % 4 == 0 and 28 + n_json + n_bin == length
    assert text.rstrip(b' ')[-1:] == b'}' and len(text) - len(text.rstrip(b' ')) < 4           # padded with spaces only
    doc = json.loads(text.decode('utf-8'))
    buf = blob[28 + n_json:]
    used = doc['buffers'][0]['byteLength']
    assert len(doc['buffers']) == 1 and 0 <= n_bin - used < 4 and not any(buf[used:])           # padded with zeros only
    return doc, buf


def accessor(doc, buf, index):
    acc = doc['accessors'][index]
    view = doc['bufferViews'][acc['bufferView']]
    dt, nc = np.dtype(DTYPES[acc['componentType']]), COMPONENTS[acc['type']]
    assert 'byteStride' not in view
    start = view['byteOffset'] + acc.get('byteOffset', 0)
    return np.frombuffer(buf, dtype=dt, count=acc['count'] * nc, offset=start).reshape(acc['count'], nc)


def check_rules(blob):
    """The structural rules; -> (document, buffer)."""
    doc, buf = parse(blob)
    assert doc['asset']['version'] == '2.0' and isinstance(doc['asset'].get('generator'), str)
    for view in doc['bufferViews']:
        assert view['byteOffset'] % 4 == 0 and view['byteOffset'] + view['byteLength'] <= doc['buffers'][0]['byteLength']
    for acc in doc['accessors']:
        view = doc['bufferViews'][acc['bufferView']]
        size = np.dtype(DTYPES[acc['componentType']]).itemsize
        off = acc.get('byteOffset', 0)
        assert off % size == 0 and (view['byteOffset'] + off) % 4 == 0 and acc['count'] >= 1
        assert off + acc['count'] * COMPONENTS[acc['type']] * size <= view['byteLength']
    prim = doc['meshes'][0]['primitives'][0]
    att = prim['attributes']
    pos = accessor(doc, buf, att['POSITION'])
    V = pos.shape[0]
    pa = doc['accessors'][att['POSITION']]
    assert pa['min'] == pos.min(0).astype(np.float64).tolist() and pa['max'] == pos.max(0).astype(np.float64).tolist()
    idx = accessor(doc, buf, prim['indices'])
    assert doc['accessors'][prim['indices']]['componentType'] == 5125 and idx.shape[0] % 3 == 0 and int(idx.max()) < V
    assert doc['bufferViews'][doc['accessors'][prim['indices']]['bufferView']]['target'] == 34963
    for name, a in att.items():
        assert doc['accessors'][a]['count'] == V and doc['bufferViews'][doc['accessors'][a]['bufferView']]['target'] == 34962, name
    col = doc['accessors'][att['COLOR_0']]
    assert col['componentType'] == 5121 and col['type'] == 'VEC4' and col['normalized'] is True
    assert (accessor(doc, buf, att['COLOR_0'])[:, 3] == 255).all()
    skin = doc['skins'][0]
    sets = sorted(k for k in att if k.startswith('JOINTS_'))
    assert sets in (['JOINTS_0'], ['JOINTS_0', 'JOINTS_1']) and all(f'WEIGHTS_{s[-1]}' in att for s in sets)
    for s in sets:
        j = doc['accessors'][att[s]]
        assert j['componentType'] == 5121 and j['type'] == 'VEC4' and int(accessor(doc, buf, att[s]).max()) < len(skin['joints'])
        w = doc['accessors'][att['WEIGHTS_' + s[-1]]]
        assert w['componentType'] == 5126 and w['type'] == 'VEC4'
    assert len(skin['joints']) == 24 == doc['accessors'][skin['inverseBindMatrices']]['count']
    assert doc['accessors'][skin['inverseBindMatrices']]['type'] == 'MAT4'
    below = set()
    todo = [skin['skeleton']]
    while todo:
        n = todo.pop()
        assert n not in below                               # a tree: no node twice
        below.add(n)
        todo += doc['nodes'][n].get('children', [])
    assert set(skin['joints']) <= below and skin['skeleton'] in skin['joints']
    for tgt in prim.get('targets', []):
        assert set(tgt) == {'POSITION'} and doc['accessors'][tgt['POSITION']]['count'] == V
        d = accessor(doc, buf, tgt['POSITION'])
        ta = doc['accessors'][tgt['POSITION']]
        assert ta['min'] == d.min(0).astype(np.float64).tolist() and ta['max'] == d.max(0).astype(np.float64).tolist()
    for anim in doc.get('animations', []):
        for ch in anim['channels']:
            sm = anim['samplers'][ch['sampler']]
            t = accessor(doc, buf, sm['input'])[:, 0]
            ta = doc['accessors'][sm['input']]
            assert (np.diff(t) > 0).all() and ta['min'] == [float(t[0])] and ta['max'] == [float(t[-1])] and t[0] >= 0
            out = accessor(doc, buf, sm['output'])
            path = ch['target']['path']
            if path == 'rotation':
                # every component is within 2^-25 of the float64 unit quaternion's: | |q|^2 - 1 | <= 2 * sum|q_i| * 2^-25 <= 2^-23
                assert sm['interpolation'] == 'LINEAR' and out.shape == (len(t), 4)
                assert np.abs((out.astype(np.float64) ** 2).sum(1) - 1.0).max() <= 2.0 ** -23 + 2.0 ** -48
            elif path == 'translation':
                assert sm['interpolation'] == 'LINEAR' and out.shape == (len(t), 3)
            else:
                assert path == 'weights' and sm['interpolation'] == 'STEP' and out.shape == (len(t) * len(prim['targets']), 1)
    return doc, buf


def _rotation(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _sample(t_keys, values, t, mode, rotation=False):
    """values [keys, n] at time t: clamped outside the keys, the key's own value at a key time."""
    t_keys = t_keys.astype(np.float64)
    v = values.astype(np.float64)
    if t <= t_keys[0]:
        return v[0]
    if t >= t_keys[-1]:
        return v[-1]
    k = int(np.searchsorted(t_keys, t, side='right')) - 1
    if mode == 'STEP' or t == t_keys[k]:
        return v[k]
    u = (t - t_keys[k]) / (t_keys[k + 1] - t_keys[k])
    if not rotation:
        return v[k] + u * (v[k + 1] - v[k])
    a, b = v[k], v[k + 1]
    d = float((a * b).sum())
    if d < 0.0:
        b, d = -b, -d
    if d > 0.9995:
        q = a + u * (b - a)
        return q / np.sqrt((q * q).sum())
    th = np.arccos(d)
    return (np.sin((1 - u) * th) * a + np.sin(u * th) * b) / np.sin(th)


def evaluate(doc, buf, t=None):
    """Vertex positions float64 [V,3] in world space at time t (seconds); None: the rest pose, no animation applied."""
    nodes = doc['nodes']
    trs = []
    for n in nodes:
        assert 'matrix' not in n and 'scale' not in n
        trs.append([np.array(n.get('translation', [0.0, 0.0, 0.0]), dtype=np.float64),
                    np.array(n.get('rotation', [0.0, 0.0, 0.0, 1.0]), dtype=np.float64)])
    mesh_node = [i for i, n in enumerate(nodes) if 'mesh' in n][0]
    morph = np.array(doc['meshes'][0].get('weights', []), dtype=np.float64)
    if t is not None:
        for anim in doc.get('animations', []):
            for ch in anim['channels']:
                sm = anim['samplers'][ch['sampler']]
                keys, out = accessor(doc, buf, sm['input'])[:, 0], accessor(doc, buf, sm['output'])
                path, node = ch['target']['path'], ch['target']['node']
                if path == 'weights':
                    assert node == mesh_node
                    morph = _sample(keys, out.reshape(len(keys), -1), float(t), sm['interpolation'])
                else:
                    trs[node][0 if path == 'translation' else 1] = _sample(keys, out, float(t), sm['interpolation'], path == 'rotation')
    local = []
    for tr, q in trs:
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = _rotation(q), tr
        local.append(m)
    parent = {c: i for i, n in enumerate(nodes) for c in n.get('children', [])}

    def glob(i):
        return local[i] if i not in parent else glob(parent[i]) @ local[i]
    prim = doc['meshes'][0]['primitives'][0]
    att = prim['attributes']
    pos = accessor(doc, buf, att['POSITION']).astype(np.float64)
    for w, tgt in zip(morph, prim.get('targets', [])):                 # morph before skin
        if w != 0.0:
            pos = pos + w * accessor(doc, buf, tgt['POSITION']).astype(np.float64)
    skin = doc['skins'][nodes[mesh_node]['skin']]
    ibm = accessor(doc, buf, skin['inverseBindMatrices']).astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)   # column-major
    mg = glob(mesh_node)
    jm = np.stack([np.linalg.inv(mg) @ glob(j) @ ibm[i] for i, j in enumerate(skin['joints'])])
    sm = np.zeros((pos.shape[0], 4, 4))
    for s in sorted(k[-1] for k in att if k.startswith('JOINTS_')):
        jn, wt = accessor(doc, buf, att['JOINTS_' + s]), accessor(doc, buf, att['WEIGHTS_' + s]).astype(np.float64)
        for k in range(4):
            sm = sm + wt[:, k, None, None] * jm[jn[:, k]]
    h = np.concatenate([pos, np.ones((pos.shape[0], 1))], 1)
    out = np.einsum('ij,vjk,vk->vi', mg, sm, h)
    return out[:, :3]


def key_times(doc, buf):
    sm = doc['animations'][0]['samplers'][0]
    return accessor(doc, buf, sm['input'])[:, 0].astype(np.float64)


# ------------------------------------------------------------------ the bounds
def rotation_defect(Rs):
    """eps = max over the matrices of ||R - U||_2, U the nearest rotation (the polar factor of R): how far the float32 bases
    the rig is written from are from rigid.  A property of the inputs."""
    R = np.asarray(Rs, dtype=np.float32).astype(np.float64).reshape(-1, 3, 3)
    u, _, vt = np.linalg.svd(R)
    return float(np.linalg.norm(R - u @ vt, ord=2, axis=(1, 2)).max())


def link_defects(Rs):
    """Of one frame's bases Rs [nb,3,3] (SMPL order): (the largest sum along a chain root .. b of D_l = ||A_l - U_l||_2, A_l =
    R_parent R_l^-1 the exact 3x3 part of the link l (A_0 = R_0^-1) and U_l the nearest rotation; the largest ||R_b^-1 -
    R_b^T||_2).  Properties of the inputs."""
    from occnerf_amd.synth import SMPL_PARENT
    R = np.asarray(Rs, dtype=np.float32).astype(np.float64).reshape(-1, 3, 3)
    inv = np.linalg.inv(R)
    A = np.stack([inv[0]] + [R[SMPL_PARENT[b]] @ inv[b] for b in range(1, R.shape[0])])
    u, _, vt = np.linalg.svd(A)
    D = np.linalg.norm(A - u @ vt, ord=2, axis=(1, 2))
    chain = D.copy()
    for b in range(1, R.shape[0]):                          # parents come first in SMPL order
        chain[b] = chain[SMPL_PARENT[b]] + D[b]
    return float(chain.max()), float(np.linalg.norm(inv - R.transpose(0, 2, 1), ord=2, axis=(1, 2)).max())


def chain_bound(Rs, reach, span, t_max, p_max, links=LONGEST_CHAIN, extra_defect=0.0):
    """The Euclidean distance allowed between evaluate() at a key time and the definition's posed = float32(sum_k w_k R_b^T (x -
    T_b)), in metres.  Rs: the frames' bases [F,nb,3,3]; reach: the largest distance between a (morphed) vertex and a joint in
    the rest pose; span: max|x| + max|T_b|; t_max: the largest stored translation component; p_max: max|posed|; extra_defect:
    the D of further links above the root (a world node), `links` counting them.

    The file holds, per joint, the chain of local transforms L_l = inv(G_parent) G_l with G_b = inv([R_b | T_b]) cnl_gtfms_b, each
    as a float32 unit quaternion and a float32 translation; the inverse bind matrices are inv(cnl_gtfms_b), pure translations
    whose float32 form is exact (the test asserts that), so G_b inv(cnl_gtfms_b) = inv([R_b | T_b]) is what the exact chain gives.
      (1) inverse against transpose.  posed uses R_b^T, the file R_b^-1, on a vector x - T_b no longer than span:
          gap span, gap = max_b ||R_b^-1 - R_b^T||_2 (link_defects).
      (2) the rotation of a link.  Its exact 3x3 part A is D away from the nearest rotation U in the 2-norm (link_defects).
          Shepperd's quaternion is the direction of a vector v that is LINEAR in the entries of A (the numerators and 4 a^2;
          the square root only scales), with ||v(U)|| = 4 a >= 2 on the branch taken and v(A) - v(U) made of sums of at most 3
          entries of A - U: ||v(A) - v(U)||_2 <= sqrt(21) D, so the unit quaternion moves by at most sqrt(21) D / 2 (1 + O(D))
          and the rotation it stands for by twice that in the 2-norm: 4.6 D.  With ||A - U|| = D the float64 quaternion's
          matrix is within 5.6 D of A.  Rounding the four components to float32 moves each by at most 2^-25, the quaternion
          by 2^-24, its matrix by 2^-23.  e_R = 5.6 D + 2^-23.
      (3) the translation of a link: each component within 2^-25 t_max: e_t = sqrt(3) 2^-25 t_max.
      (4) along a chain the transforms are rigid up to 1 + O(D), so the errors add: every link's e_R acts on a vector from
          its joint to the vertex, no longer than reach: reach (5.6 sum_l D_l + links 2^-23) + links e_t, the sum of D_l the
          largest any chain has (link_defects), over the frames.
      (5) the weights are the same numbers on both sides and sum to at most 1 + 8 * 2^-25.
      (6) posed is rounded to float32: sqrt(3) 2^-25 p_max.  The float64 evaluation itself: 1e-12.
    A factor 1.01 covers the second-order terms (the D are of the order 1e-5, the gap 1e-4)."""
    per_frame = [link_defects(R) for R in np.asarray(Rs, dtype=np.float32).reshape((-1,) + np.asarray(Rs).shape[-3:])]
    chain, gap = max(c for c, _ in per_frame) + extra_defect, max(g for _, g in per_frame)
    e_t = np.sqrt(3.0) * 2.0 ** -25 * t_max
    return 1.01 * (1 + 2.0 ** -22) * (reach * (5.6 * chain + links * 2.0 ** -23) + links * e_t + gap * span) \
        + np.sqrt(3.0) * 2.0 ** -25 * p_max + 1e-12


def corrective_bound(M, d32, target):
    """Per vertex, the largest |p + M float64(d32) - target| by component, p, M and d the definition's float64 numbers: d32 is d
    with every component rounded once to float32, |d32 - d| <= 2^-24 |d| by component, carried through M: ||M||_inf 2^-24 ||d||_inf
    (||d32|| (1 + 2^-23) stands for ||d||); the float32 rounding of the target the issue asks to allow: 2^-24 ||target||_inf; and the
    float64 solve itself (M is a blend of rotations, well conditioned): 2^-44 (||target||_inf + ||M||_inf ||d||_inf)."""
    norm = np.abs(M).sum(-1).max(-1)
    d = np.abs(np.asarray(d32, dtype=np.float64)).max(-1) * (1 + 2.0 ** -23)
    t = np.abs(np.asarray(target, dtype=np.float64)).max(-1)
    return norm * 2.0 ** -24 * d + 2.0 ** -24 * t + 2.0 ** -44 * (t + norm * d)
