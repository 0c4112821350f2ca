"""The item tables the trainable heads' flat buffers are built from (implementation_phd_lab_vision_amd/trainable.py): the layout each
gives against the one the heads uploaded before the tables existed (tests/golden/train_launch_sequences.json, recorded on the device),
their reference keys against the optimizer's parameter names, and the reference-layout round trip with its zero padding."""
import json

import pytest
import torch

from implementation_phd_lab_vision_amd import train, train_ar, train_joint, trainable
from implementation_phd_lab_vision_amd.model import expected_keys
from tests.helpers import GOLDEN

FIXTURE = json.loads((GOLDEN / "train_launch_sequences.json").read_text())
DIMS = ((64, 17, 1), (1024, 17, 2))
KINDS = ("phase1", "phase2", "joint")


def items_of(kind, number_blocks):
    return {"phase1": lambda: train.phase1_items(number_blocks), "phase2": train_ar.ar_items,
            "joint": lambda: train_joint.joint_items(number_blocks)}[kind]()


def names_of(kind, number_blocks):
    return {"phase1": lambda: train.trainable_names(number_blocks), "phase2": train_ar.ar_trainable_names,
            "joint": lambda: train_joint.joint_trainable_names(number_blocks)}[kind]()


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: ",".join(map(str, d)))
@pytest.mark.parametrize("kind", KINDS)
def test_layout_equals_recorded(kind, dims):
    layout = trainable.flat_layout(items_of(kind, dims[2]), expected_keys(*dims))
    assert [[n, o, list(s)] for n, o, s in layout] == FIXTURE["layouts"][kind][",".join(map(str, dims))]


@pytest.mark.parametrize("kind", KINDS)
def test_reference_keys_are_the_trainable_names(kind):
    items = items_of(kind, 1)
    keys = [key for _, key, _ in items]
    assert len(set(keys)) == len(keys) and len({name for name, _, _ in items}) == len(items)
    assert set(keys) == set(names_of(kind, 1))


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_identity_outside_padding_zero_inside(kind):
    dims = (64, 17, 1)
    items, shapes = items_of(kind, dims[2]), expected_keys(*dims)
    layout = trainable.flat_layout(items, shapes)
    total = layout[-1][1] + int(torch.Size(layout[-1][2]).numel())
    g = torch.Generator().manual_seed(7)
    flat = torch.randn(total, generator=g)                              # nonzero in the padding too
    named = trainable.unpack_flat(items, shapes, flat)
    assert {k: tuple(v.shape) for k, v in named.items()} == {key: shapes[key] for _, key, _ in items}
    back = trainable.pack_flat(items, shapes, named, torch.zeros(total))
    again = trainable.unpack_flat(items, shapes, back)
    assert all(torch.equal(named[k], again[k]) for k in named)
    n_ref = sum(v.numel() for v in named.values())
    same = back == flat
    assert int(same.sum()) == n_ref and int((back != 0).sum()) == n_ref    # identity on the reference's entries ...
    assert torch.all(back[~same] == 0) and int((~same).sum()) == total - n_ref          # ... zeros in the GEMM padding
    for (name, key, kind_), (_, off, shape) in zip(items, layout):
        entry = back[off: off + int(torch.Size(shape).numel())].view(shape)
        if kind_ == "conv":                                             # (d, d, 3) -> (d, 3d): column k*d + c holds weight[:, c, k]
            assert torch.equal(entry.view(64, 3, 64)[:, 2, :], named[key][:, :, 2])
        elif kind_ == "pad_cols":
            assert torch.equal(entry[:, : shapes[key][1]], named[key]) and not entry[:, shapes[key][1]:].any()
        elif kind_ == "pad_rows":
            assert torch.equal(entry[: shapes[key][0]], named[key]) and not entry[shapes[key][0]:].any()
    bad = dict(named)
    key = items[0][1]
    bad[key] = torch.zeros(3, 5)
    with pytest.raises(ValueError, match=f"{key}: shape \\(3, 5\\), expected"):
        trainable.pack_flat(items, shapes, bad, torch.zeros(total))
