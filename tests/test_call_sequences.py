"""The call sequences of tests/test_gpu_call_sequences.py without a device: the model alone must reach every cache transition the
GPU cases are named after, and the two functions that build the keys of the launch-plan caches must tell apart exactly what a
plan holds."""

import numpy as np
import pytest

import call_sequences as CS
import test_gpu_call_sequences as T


class Stand:
    """An array as far as a key function looks at it."""

    def __init__(self, ptr, shape=(8, 6, 4), strides=(8, 64, 384)):
        self.ptr, self.shape, self.strides = ptr, shape, strides


# ---- census ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.OBJECTS)
def test_the_sequences_of_an_object_reach_every_transition(name, tmp_path):
    spec = T.build(name, tmp_path)[2]
    seqs = T.sequences(spec)
    got = CS.census(spec, seqs)
    assert got["steps"] == len(T.SEEDS) * T.LENGTH
    few = {k: n for k, n in got["kinds"].items() if n < 3}
    assert not few, f"{name}: step kinds reached fewer than 3 times: {few}\n{got}"
    few = {k: n for k, n in got["causes"].items() if n < 3}
    assert not few, f"{name}: causes of a miss reached fewer than 3 times: {few}\n{got}"
    few = {k: n for k, n in got["paths"].items() if n < 3}
    assert not few, f"{name}: call paths taken fewer than 3 times: {few}"
    assert 3 * got["hits"] >= got["steps"], f"{name}: {got['hits']} hits in {got['steps']} steps"
    never = [k for k, n in got["hit after"].items() if n < 1]
    assert not never, f"{name}: no hit directly after a miss for {never}\n{got}"
    assert 2 * got["may miss"] <= got["hits"], f"{name}: {got['may miss']} of {got['hits']} hits are left to the fix"
    # the palette's pairs, for the objects whose plans hold a float scalar
    if spec.generic and spec.float_params:
        p, dt = next(iter(spec.float_params.items()))
        zeros = sum(1 for steps in seqs for a, b in zip(steps, steps[1:]) if not b.refused and b.cause == "scalar bits"
                    and {CS.scalar_bits(dt, a.scalars[p]), CS.scalar_bits(dt, b.scalars[p])} == {CS.scalar_bits(dt, 0.0), CS.scalar_bits(dt, -0.0)})
        assert zeros >= 1, f"{name}: no call with 0.0 directly after one with -0.0 or the other way round"


def test_the_sequences_are_reproducible(tmp_path):
    spec = T.build("local_f64", tmp_path)[2]
    assert T.sequences(spec) == T.sequences(spec)


def test_the_model_tells_a_hit_from_each_cause():
    spec = CS.Spec("toy", ("a", "out"), T.DOMAINS, {"s": "float64"}, {}, True, True)
    model = CS.Model(spec)
    base = CS.Step("repeat", "call", 0, T.DOMAINS[0], {"a": 0, "out": 0}, {"a": 0, "out": 0}, {"s": 0.0})

    def call(**changes):
        step = CS.dataclasses.replace(base, **changes)
        model.call(step)
        return step.hit, step.cause

    assert call() == (False, "cold")
    assert call() == (True, None)
    assert call(scalars={"s": -0.0}) == (False, "scalar bits")
    assert call(scalars={"s": 0}) == (True, None)  # 0 and False are 0.0 in a float64 parameter
    assert call(origin={"a": 1, "out": 0}) == (False, "origin")
    assert call(stream=3) == (False, "stream")
    model.mutate("repoint", "a", 0, 1)
    assert call() == (False, "address")
    model.mutate("repitch", "a", 0, 2)
    assert call() == (False, "strides")
    model.mutate("repoint", "a", 0, 0)
    hit = CS.dataclasses.replace(base)
    model.call(hit)
    assert hit.hit and hit.may_miss  # the first entry again, stale in between
    model.mutate("replace", "a", 0, 0)
    assert call() == (False, "dead object")
    assert call(domain=T.DOMAINS[1]) == (False, "domain")  # ... which takes the scratch of stream 0 to another domain
    assert call() == (False, "scratch eviction")


# ---- the domains -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["local_f64", "local_f32", "two_stage_written_input", "two_sweep_0"])
def test_the_domains_reach_a_lane_twin_a_point_twin_and_several_workgroups(name, tmp_path):
    _, hip, spec, *_ = T.build(name, tmp_path)
    labels, groups = T.twins_reached(hip, spec.domains)
    assert "point" in labels, labels
    if name == "two_sweep_0":
        assert any(label.startswith("tc") for label in labels), labels
    elif name == "two_stage_written_input":
        assert labels & {"vec", "vecs"}, labels
    else:  # its conditional statements leave the local stencil without 16-byte-lane twins
        assert not any(k.vec for k in type(hip)._gt_program_.kernels)
    assert groups > 1


def test_the_local_stencil_keeps_a_temporary_in_scratch_and_the_library_objects_are_bound(tmp_path):
    from gt4py_amd.cartesian.backend import hip_backend

    for name in ("local_f64", "local_f32", "two_stage_written_input"):
        assert type(T.build(name, tmp_path)[1])._gt_program_.plan.scratch, name
    for name in ("lap5_f32", "lap5_f64", "hdiff_field", "hdiff_scalar", "tridiag"):
        assert isinstance(T.build(name, tmp_path)[1], hip_backend.HipStencilObject), name


# ---- the key functions -------------------------------------------------------------------------------------------------------------
def generic_key(value, dtype="float64", array=None):
    from gt4py_amd.cartesian.backend import hip_generic

    array = array or Stand(0x7F00_0000_0000)
    return hip_generic.launch_key(0, (8, 6, 4), [array], [(0, 0, 0)], [np.dtype(dtype)], [value]), array


def test_scalars_are_keyed_by_their_bits_in_the_dtype_of_the_parameter():
    a = Stand(0x7F00_0000_0000)
    key = lambda v, dt="float64": generic_key(v, dt, a)[0]  # noqa: E731
    assert key(0.0) != key(-0.0)
    assert key(float("nan")) == key(float("nan")) == key(np.nan)
    assert key(1) == key(1.0) == key(True) == key(np.float32(1.0))
    assert key(0.1, "float32") == key(np.float32(0.1), "float32")
    assert key(0.1) != key(np.float32(0.1))
    assert key(1, "int64") == key(True, "int64") != key(0, "int64")
    assert hash(key(0.0)) is not None


def test_arrays_are_keyed_by_object_address_shape_and_strides():
    from gt4py_amd.cartesian.backend import hip_backend

    a = Stand(0x7F00_0000_0000)
    for key in (lambda: generic_key(1.5, array=a)[0], lambda: hip_backend.launch_key((8, 6, 4), [a], [(0, 0, 0)])):
        first = key()
        assert key() == first
        a.ptr += 1 << 20
        moved = key()
        assert moved != first
        a.strides = (8, 128, 768)
        pitched = key()
        assert pitched != moved
        a.shape = (8, 6, 3)
        assert key() != pitched
        a.ptr, a.shape, a.strides = 0x7F00_0000_0000, (8, 6, 4), (8, 64, 384)
        assert key() == first
        b = Stand(a.ptr, a.shape, a.strides)
        a_key = key()
        a, b = b, a
        assert key() != a_key  # another object at the same place
        a, b = b, a


def test_an_unhashable_scalar_means_do_not_cache():
    with pytest.raises(TypeError):
        generic_key(np.array(1.0))
    with pytest.raises(TypeError):
        generic_key([1.0])
