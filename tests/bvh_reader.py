"""A small BVH reader and forward kinematics in numpy fp64, written from the format's description alone (HIERARCHY of ROOT / JOINT /
End Site blocks with OFFSET and CHANNELS, then MOTION): what tests/test_kinematics_cpu.py and tests/test_kinematics_gpu.py read the
product's files back with.  Nothing in the product imports this file."""
import numpy as np


def parse(text):
    """Returns a dict: ``names`` [J] in file order, ``parent`` [J] (-1 at the root), ``offset`` (J, 3), ``channels`` [J] lists of channel
    names, ``end_sites`` {joint: offset}, ``frames``, ``frame_time`` and ``motion`` (frames, total channels)."""
    tok = text.split()
    pos = 0

    def take():
        nonlocal pos
        pos += 1
        return tok[pos - 1]

    def expect(word):
        got = take()
        assert got == word, f"expected {word!r}, got {got!r} at token {pos - 1}"

    names, parent, offset, channels, end_sites = [], [], [], [], {}
    expect("HIERARCHY")

    def node(kind, up):
        assert kind in ("ROOT", "JOINT")
        k = len(names)
        names.append(take())
        parent.append(up)
        expect("{")
        expect("OFFSET")
        offset.append([float(take()) for _ in range(3)])
        expect("CHANNELS")
        channels.append([take() for _ in range(int(take()))])
        while True:
            word = take()
            if word == "}":
                return
            if word == "End":
                expect("Site")
                expect("{")
                expect("OFFSET")
                end_sites[k] = [float(take()) for _ in range(3)]
                expect("}")
            else:
                node(word, k)

    node(take(), -1)
    expect("MOTION")
    expect("Frames:")
    frames = int(take())
    expect("Frame")
    expect("Time:")
    frame_time = float(take())
    values = np.array([float(v) for v in tok[pos:]], dtype=np.float64)
    total = sum(len(c) for c in channels)
    assert values.size == frames * total, f"{values.size} motion values for {frames} frames of {total} channels"
    return dict(names=names, parent=parent, offset=np.array(offset), channels=channels, end_sites=end_sites, frames=frames,
                frame_time=frame_time, motion=values.reshape(frames, total))


def _axis_rotation(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    if axis == "X":
        return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    if axis == "Y":
        return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def forward_kinematics(bvh):
    """World positions (frames, J, 3) in file order: a joint's rotation is the product of its rotation channels in channel order, its
    position its parent's position plus the parent's global rotation times OFFSET (the root: OFFSET plus its position channels)."""
    j = len(bvh["names"])
    out = np.zeros((bvh["frames"], j, 3))
    for f in range(bvh["frames"]):
        at, glob = 0, [None] * j
        for k in range(j):
            local, trans = np.eye(3), np.zeros(3)
            for ch in bvh["channels"][k]:
                v = bvh["motion"][f, at]
                at += 1
                if ch.endswith("position"):
                    trans["XYZ".index(ch[0])] = v
                else:
                    assert ch.endswith("rotation")
                    local = local @ _axis_rotation(ch[0], v)
            up = bvh["parent"][k]
            if up < 0:
                out[f, k], glob[k] = bvh["offset"][k] + trans, local
            else:
                out[f, k], glob[k] = out[f, up] + glob[up] @ bvh["offset"][k] + trans, glob[up] @ local
    return out
