"""tests/scene_edits.py, the harness every scene-edit GPU test goes through, pinned on the CPU: its array assertions over
a stand-in renderer that serves scene_counts() and scene_array() from numpy arrays, made from a host-built desc with the
device's leaf boxes filled in by a restatement of its own (mesh_add_cases' neg_zero and pool_tail between the add and
the spawn: an instanced quad, pooled meshes nobody registered, an added mesh that no instance carries); its seeded rays
by a digest."""
import hashlib

import numpy as np
import pytest

import mesh_add_cases as ac
from instance_set_cases import desc_counts
from parity import host_scene_array
from scene_edits import (ELEM_DT, INST_DT, PRIM_DT, assert_mesh_arrays, assert_scene_is, device_arrays, device_max,
                         device_min, seeded_rays)

LEAF = 0x80000000
NAMES = ("neg_zero", "pool_tail")


def test_device_min_max_restate_the_sign_of_zero():
    p = np.array([[[0.0, -0.0, 1.0], [-0.0, -0.0, 2.0], [0.0, -0.0, 0.0]]], np.float32)
    assert device_min(p).view(np.uint32).tolist() == [[0x80000000, 0x80000000, 0]]
    assert device_max(p).view(np.uint32).tolist() == [[0, 0x80000000, 0x40000000]]


def _signed_order(p):
    """The corners as float64 keys that order -0 below +0, as the device's fminf / fmaxf do."""
    key = p.astype(np.float64)
    key[p.view(np.uint32) == LEAF] = -1e-300
    return key


def _fill_leaves(desc, arrays, slices):
    """The device's leaf boxes in arrays[2] for the mesh slices given: per axis the corner that is least / greatest."""
    corners = np.frombuffer(host_scene_array(desc, 1, PRIM_DT).tobytes(), np.float32).reshape(-1, 3, 4)[:, :, :3]
    for _, prim, n0, nc in slices:
        for node in arrays[2][n0: n0 + nc]:
            if node["entry"] >= LEAF:
                tri = np.ascontiguousarray(corners[prim + int(node["entry"] - LEAF)])
                key = _signed_order(tri)
                node["min"] = np.take_along_axis(tri, key.argmin(axis=0)[None], 0)[0]
                node["max"] = np.take_along_axis(tri, key.argmax(axis=0)[None], 0)[0]


class Standin:
    """scene_counts() and scene_array(idx, dt, n) over what the device holds for a host-built desc: the asset nodes'
    leaves of the instanced and the `registered` slices with their triangle's box, the TLAS's with their instance's."""

    def __init__(self, desc, registered=()):
        self.arrays = [host_scene_array(desc, i, ELEM_DT[i]).copy() for i in range(9)]
        inst = np.frombuffer(self.arrays[4].tobytes(), np.uint32).reshape(-1, 44)
        _fill_leaves(desc, self.arrays, {tuple(int(v) for v in row[40:44]) for row in inst} | set(registered))
        boxes = inst.view(np.float32)
        for node in self.arrays[5]:
            if node["entry"] >= LEAF:
                node["min"], node["max"] = boxes[node["entry"] - LEAF, 0:3], boxes[node["entry"] - LEAF, 4:7]
        self.counts = desc_counts(desc)

    def scene_counts(self):
        return list(self.counts)

    def scene_array(self, idx, dt, n):
        assert dt == ELEM_DT[idx]
        if n < self.counts[idx]:
            raise RuntimeError("hk_read_scene_array failed (-1): destination too small")  # as the device refuses
        return np.concatenate([self.arrays[idx][:self.counts[idx]], np.zeros(n - self.counts[idx], dt)])

    def words(self, idx):
        return self.arrays[idx].view(np.uint32).reshape(-1)


def _made(name):
    """(desc, the added mesh's slices, a stand-in that holds them registered) of the case between add and spawn."""
    desc, registered = ac.add_only(name, 1).desc, ac.new_slices(name, 1)
    return desc, registered, Standin(desc, registered)


def _leaf_words(r, idx, slices=None):
    """Indices into r.words(idx) of the box words (min xyz, max xyz) of array idx's leaves, those of `slices` only."""
    nodes = r.arrays[idx]
    inside = np.zeros(len(nodes), bool)
    for _, _, n0, nc in [(0, 0, 0, len(nodes))] if slices is None else slices:
        inside[n0: n0 + nc] = True
    rows = np.flatnonzero((nodes["entry"] >= LEAF) & inside)
    return (rows[:, None] * 8 + np.array([0, 1, 2, 4, 5, 6])).reshape(-1)


@pytest.mark.parametrize("name", NAMES)
def test_the_device_image_of_a_host_scene_passes(name):
    desc, registered, r = _made(name)
    assert_scene_is(r, desc, registered)
    assert device_arrays(r) == [a.tobytes() for a in r.arrays]
    assert [len(b) for b in device_arrays(r, (2, 4))] == [32 * r.counts[2], INST_DT.itemsize * r.counts[4]]


@pytest.mark.parametrize("name", NAMES)
def test_one_flipped_bit_in_any_array_fails_naming_it(name):
    desc, registered, _ = _made(name)
    for idx in range(9):
        for word in (0, -1):
            r = Standin(desc, registered)
            r.words(idx)[word] ^= 4
            with pytest.raises(AssertionError, match=f"array {idx}"):
                assert_scene_is(r, desc, registered)
    for idx in (2, 5):  # and in a leaf's box, where the device's node is not the host's
        r = Standin(desc, registered)
        r.words(idx)[_leaf_words(r, idx)[-1]] ^= 1
        with pytest.raises(AssertionError, match=f"array {idx}: leaf boxes"):
            assert_scene_is(r, desc, registered)


def test_a_leaf_box_zero_of_the_other_sign_fails():
    desc, registered, r = _made("neg_zero")
    at = _leaf_words(r, 2, registered)
    zeros = at[(r.words(2)[at] & 0x7FFFFFFF) == 0]
    assert {int(w) for w in r.words(2)[zeros]} == {0, LEAF}  # (the case: zeros of both signs in the leaf boxes)
    for sign in (0, LEAF):
        r = Standin(desc, registered)
        r.words(2)[zeros[r.words(2)[zeros] == sign][0]] ^= LEAF
        with pytest.raises(AssertionError, match="array 2: leaf boxes"):
            assert_scene_is(r, desc, registered)


@pytest.mark.parametrize("name", NAMES)
def test_a_count_changed_by_one_fails_naming_it(name):
    desc, registered, _ = _made(name)
    for idx in range(9):
        r = Standin(desc, registered)
        r.counts[idx] -= 1
        with pytest.raises(AssertionError, match=rf"counts of arrays \[{idx}\]"):
            assert_scene_is(r, desc, registered)
    r = Standin(desc, registered)
    r.counts[1] -= 1
    with pytest.raises(AssertionError, match="counts of arrays 0-2"):
        assert_mesh_arrays(r, desc, registered)


@pytest.mark.parametrize("name", NAMES)
def test_registered_slices_carry_boxes_and_unregistered_ones_are_empty(name):
    desc, registered, r = _made(name)
    assert_scene_is(Standin(desc), desc)  # nobody registered the added mesh: its leaves are the host's, empty
    with pytest.raises(AssertionError, match="array 2: leaf boxes"):
        assert_scene_is(Standin(desc), desc, registered)  # registered, and its leaves were left empty
    with pytest.raises(AssertionError, match="array 2: leaf boxes"):
        assert_scene_is(r, desc)  # not registered, and its leaves were filled


def test_pooled_meshes_nobody_registered_have_empty_leaves():
    name = "pool_tail"
    desc, registered, r = _made(name)
    scene = ac.add_only(name, 1)
    pooled = [scene.mesh_index(i) for i in (1, 2)]
    assert not set(pooled) & (set(registered) | {scene.mesh_index(0)})
    at = _leaf_words(r, 2, pooled)
    host = host_scene_array(desc, 2, ELEM_DT[2]).view(np.uint32).reshape(-1)
    assert len(at) and np.array_equal(r.words(2)[at], host[at])
    _fill_leaves(desc, r.arrays, pooled)
    assert (r.words(2)[at] != host[at]).any()
    with pytest.raises(AssertionError, match="array 2: leaf boxes"):
        assert_scene_is(r, desc, registered)
    assert_scene_is(r, desc, registered + pooled)


@pytest.mark.parametrize("name", NAMES)
def test_longer_arrays_accept_a_tail_and_reject_a_changed_head(name):
    desc, registered, r = _made(name)
    with pytest.raises(AssertionError, match="counts of arrays 0-2"):
        assert_mesh_arrays(r, desc, registered, longer=True)  # nothing was appended
    rng = np.random.default_rng(7)
    for idx in range(3):
        tail = np.frombuffer(rng.bytes(3 * ELEM_DT[idx].itemsize), ELEM_DT[idx])
        r.arrays[idx] = np.concatenate([r.arrays[idx], tail])
        r.counts[idx] += 3
    assert_mesh_arrays(r, desc, registered, longer=True)
    with pytest.raises(AssertionError, match="counts of arrays 0-2"):
        assert_mesh_arrays(r, desc, registered)
    for idx in range(3):
        head = desc_counts(desc)[idx] * ELEM_DT[idx].itemsize // 4
        r.words(idx)[head - 1] ^= 2
        with pytest.raises(AssertionError, match=f"array {idx}"):
            assert_mesh_arrays(r, desc, registered, longer=True)
        r.words(idx)[head - 1] ^= 2
        r.words(idx)[head] ^= 2  # the tail's first word: not the host's to say
        assert_mesh_arrays(r, desc, registered, longer=True)


def test_seeded_rays_are_the_rays_the_tests_traced_before_the_harness():
    """The digest is of the rays, early and excl arrays that test_traced_rays_after_the_update_equal_a_fresh_context of
    tests/test_gpu_mesh_update.py built inline (mesh_cases.SEED, shared_mesh's six instances) before seeded_rays took
    the block over: computed once from that block, copied out as it stood."""
    rays, early, excl = seeded_rays(0x4D455348, 6)
    assert (rays.dtype, early.dtype, excl.dtype) == (np.float32, np.float32, np.uint32)
    assert (rays.shape, early.shape, excl.shape) == ((256, 6), (256,), (256,))
    digest = hashlib.sha256(rays.tobytes() + early.tobytes() + excl.tobytes()).hexdigest()
    assert digest == "00a0fb20d3c92304c93c9dbf21543b8c44a05b21ff6c3e275c9d4b6245f7004a"
    taller = seeded_rays(0x4D455348, 6, top=3.0)
    assert np.array_equal(taller[0][:, :3], rays[:, :3]) and not np.array_equal(taller[0][:, 3:], rays[:, 3:])
