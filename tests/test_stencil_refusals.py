"""The refusals of the stencil entries (``gt4mi_lap5_*``, ``gt4mi_lap5_ring_*``, ``gt4mi_hdiff_*``, ``gt4mi_hdiff_ring_*``), byte for
byte, without a GPU -- the replay of tests/test_refusal_messages.py for the entries whose argument preparation lives in
csrc/lap5.hip.h (``lap5_views``, ``lap5_with_variant``) and csrc/hdiff.hip.h (``hdiff_views``).

What a call is refused with -- return code and the bytes of ``gt4mi_last_error()`` --, WHICH refusal wins when several apply, and
which calls return ``GT4MI_OK`` for an empty domain before anything else is looked at is behaviour;
tests/golden/stencil_refusals.json records it for a generated table: per field role the mutations ``make_view`` refuses (no
descriptor, no data, a stride that is no multiple of the item size, an origin below the reach, a shape one short, along each axis),
then unknown variants, overlaps, every width rule of the two ring entries, null / negative / oversized / empty domains, and pairs of
these that pin the order of the checks.

These entries have no dry-run flag, and every call carries made-up device addresses.  So the table may hold only calls that return
before the first HIP runtime call: refusals, and accepted calls whose domain is empty along at least one axis.  ``_guard`` asserts
that of the fixture, in the recorder and in the test.

The fixture is recorded from a build of the commit BEFORE a change to these entries, never from the code under test:

    python tests/test_stencil_refusals.py --record      # in a tree of the parent commit, after build()
"""

import copy
import ctypes
import json
import pathlib
import sys

if __name__ == "__main__":
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from gt4py_amd import _lib
from test_refusal_messages import AXES, Entry, _i64, _one

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "stencil_refusals.json"
LAP5_WHY = "every point reads its neighbours' OLD values"  # the long overlap text of gt4mi_lap5_* and gt4mi_hdiff_*


def _i32(values):
    return None if values is None else (ctypes.c_int * len(values))(*values)


class Stencil(Entry):
    """One field per role, shape (8, 8, 4) I-contiguous, origin (2, 2, 0); the domain is 4 x 4 x 4."""

    reach = 0  # of the first role, along I and J

    def __init__(self, name, symbol, size, flags=0):
        self.name, self.symbol, self.size, self.flags = name, symbol, size, flags

    def base(self, n=1):
        s = self.size
        state = {role: [{"ptr": (r + 1) * 0x100000, "shape": [8, 8, 4], "strides": [s, 8 * s, 64 * s], "origin": [2, 2, 0]}]
                 for r, (role, _, _) in enumerate(self.roles)}
        state["extent"] = [4, 4, 4]
        return state

    def box(self, state, role):
        r = self.reach if role == self.roles[0][0] else 0
        return list(state["extent"]), [r, r, 0], [r, r, 0]

    def call(self, *args):
        return getattr(_lib.load(), self.symbol)(*args, None, None)  # stream 0, no exec info


class Lap5(Stencil):
    roles = (("inp", False, ()), ("out", True, ()))
    reach = 1

    def base(self, n=1):
        state = super().base()
        state["variant"] = _lib.LAP_DOCS
        return state

    def run(self, s):
        return self.call(_i64(s["extent"]), _one(s["inp"]), _one(s["out"]), s["variant"], self.flags)


class Lap5Ring(Lap5):
    def base(self, n=1):
        state = super().base()
        state.update(outer=[1, 1, 1, 1], inner=[1, 1, 1, 1])
        return state

    def box(self, state, role):
        """The domain grown by ``outer`` (W, E, S, N), which ``inp`` is read one point beyond."""
        o, r = state["outer"], 1 if role == "inp" else 0
        return list(state["extent"]), [o[0] + r, o[2] + r, 0], [o[1] + r, o[3] + r, 0]

    def run(self, s):
        return self.call(_i64(s["extent"]), _one(s["inp"]), _one(s["out"]), s["variant"], self.flags, _i32(s["outer"]), _i32(s["inner"]))


class Hdiff(Stencil):
    roles = (("in_field", False, ()), ("out_field", True, ()), ("coeff", False, ()))
    reach = 2

    def run(self, s):
        return self.call(_i64(s["extent"]), _one(s["in_field"]), _one(s["out_field"]), _one(s["coeff"]), 0.25, self.flags)


class HdiffRing(Hdiff):
    def base(self, n=1):
        state = super().base()
        state["widths"] = [1, 1, 1, 1]
        return state

    def run(self, s):
        return self.call(_i64(s["extent"]), _one(s["in_field"]), _one(s["out_field"]), _one(s["coeff"]), 0.25, self.flags, _i32(s["widths"]))


LAP5 = (Lap5("lap5_f64", "gt4mi_lap5_f64", 8), Lap5("lap5_f32", "gt4mi_lap5_f32", 4),
        Lap5("lap5_f32_literal32", "gt4mi_lap5_f32", 4, _lib.LAP_LITERAL_F32))
LAP5_RING = (Lap5Ring("lap5_ring_f64", "gt4mi_lap5_ring_f64", 8), Lap5Ring("lap5_ring_f32", "gt4mi_lap5_ring_f32", 4),
             Lap5Ring("lap5_ring_f32_literal32", "gt4mi_lap5_ring_f32", 4, _lib.LAP_LITERAL_F32))
HDIFF = (Hdiff("hdiff_f64", "gt4mi_hdiff_f64", 8), Hdiff("hdiff_f32", "gt4mi_hdiff_f32", 4, _lib.HDIFF_LIMITER))
HDIFF_RING = (HdiffRing("hdiff_ring_f64", "gt4mi_hdiff_ring_f64", 8, _lib.HDIFF_LIMITER),
              HdiffRing("hdiff_ring_f32", "gt4mi_hdiff_ring_f32", 4, _lib.HDIFF_INTERNAL_F32 | _lib.HDIFF_COEFF_F32))
ENTRIES = LAP5 + LAP5_RING + HDIFF + HDIFF_RING


def _break(entry, state, role):
    """The simplest refusal of ``role``: no data."""
    state[role][0]["ptr"] = 0


def _same(state, a, b, rows=0):
    """Field ``b`` becomes field ``a`` moved up by ``rows`` rows."""
    fa, fb = state[a][0], state[b][0]
    fb.update(copy.deepcopy(fa))
    fb["ptr"] += rows * fa["strides"][1]


def _field_cases(entry, role):
    def variant(name):
        state = entry.base()
        return f"{entry.name}/{role}/{name}", state, state[role][0]

    # no descriptor at all -- not for coeff (that is a call with a scalar coefficient: accepted, it would launch) and not for
    # gt4mi_lap5_ring_*, which copies both descriptors before it looks at them (a null pointer there is a crash, not a refusal)
    if role != "coeff" and entry not in LAP5_RING:
        name, state, _ = variant("absent")
        state[role] = None
        yield name, state
    name, state, f = variant("null")
    f["ptr"] = 0
    yield name, state
    for ax in AXES:
        name, state, f = variant(f"ax{ax}/stride+half")
        f["strides"][ax] += entry.size // 2
        yield name, state
        extent, lo, hi = entry.box(state, role)
        for origin in sorted({-1, lo[ax] - 1}):
            name, state, f = variant(f"ax{ax}/origin={origin}")
            f["origin"][ax] = origin
            yield name, state
        name, state, f = variant(f"ax{ax}/shape=need-1")
        f["shape"][ax] = f["origin"][ax] + extent[ax] + hi[ax] - 1
        yield name, state
        name, state, f = variant(f"ax{ax}/origin={lo[ax]}/shape=need-1")  # at the lowest origin that passes
        f["origin"][ax] = lo[ax]
        f["shape"][ax] = lo[ax] + extent[ax] + hi[ax] - 1
        yield name, state
    # two fields at once: the earlier role is reported
    for other, _, _ in entry.roles:
        if other != role:
            name, state, _ = variant(f"null+{other}-null")
            _break(entry, state, role)
            _break(entry, state, other)
            yield name, state


def _domain_cases(entry):
    first, second = entry.roles[0][0], entry.roles[1][0]

    def variant(name):
        state = entry.base()
        for key in ("inner", "widths"):  # (of the ring entries: they have to fit an empty domain; _width_cases has the others)
            if key in state and "=0" in name:
                state[key] = [0, 0, 0, 0]
        return f"{entry.name}/domain/{name}", state

    name, state = variant("null")
    state["extent"] = None
    yield name, state
    for ax in AXES:
        for value in (-1, 2 ** 31):
            name, state = variant(f"ax{ax}={value}")
            state["extent"][ax] = value
            yield name, state
        name, state = variant(f"ax{ax}=-1+{first}-null")
        state["extent"][ax] = -1
        _break(entry, state, first)
        yield name, state
        # an empty domain: accepted -- after the fields have been looked at or before (lap5 ring), but before any overlap
        name, state = variant(f"ax{ax}=0")
        state["extent"][ax] = 0
        yield name, state
        name, state = variant(f"ax{ax}=0+{second}-null")
        state["extent"][ax] = 0
        _break(entry, state, second)
        yield name, state
        name, state = variant(f"ax{ax}=0+{second}-is-{first}")
        state["extent"][ax] = 0
        _same(state, first, second)
        yield name, state
    name, state = variant("all=0")
    state["extent"] = [0, 0, 0]
    yield name, state


def _overlap_cases(entry):
    first, second = entry.roles[0][0], entry.roles[1][0]

    def variant(name):
        state = entry.base()
        return f"{entry.name}/overlap/{name}", state

    for rows in (0, 2):
        name, state = variant(f"{second}-is-{first}+{rows}-rows")
        _same(state, first, second, rows)
        yield name, state
    if entry in HDIFF + HDIFF_RING:
        # (coeff as the SAME elements as out_field is accepted and would launch; moved by two rows it is refused)
        name, state = variant("coeff-is-out_field+2-rows")
        _same(state, "out_field", "coeff", 2)
        yield name, state
        name, state = variant("coeff-is-out_field+half-an-item")
        _same(state, "out_field", "coeff")
        state["coeff"][0]["ptr"] += entry.size // 2
        yield name, state
        name, state = variant("out_field-is-in_field+coeff-is-out_field+2-rows")  # in / out is reported first
        _same(state, "in_field", "out_field")
        _same(state, "out_field", "coeff", 2)
        yield name, state
    if entry in LAP5 + LAP5_RING:
        name, state = variant(f"{second}-is-{first}+variant=99")  # the overlap is reported, not the variant
        _same(state, first, second)
        state["variant"] = 99
        yield name, state


def _variant_cases(entry):
    for value in (-1, 4, 99):
        state = entry.base()
        state["variant"] = value
        yield f"{entry.name}/variant={value}", state
    state = entry.base()
    state["variant"] = 4
    _break(entry, state, "out")
    yield f"{entry.name}/variant=4+out-null", state  # the field is reported


def _width_cases(entry, keys):
    """Every width rule of a ring entry, alone, with an empty domain and with a bad field."""
    first = entry.roles[0][0]

    def mutations():
        for key in keys:
            yield f"{key}-null", lambda s, key=key: s.update({key: None})
            for side in range(4):
                yield f"{key}[{side}]=-1", lambda s, key=key, side=side: s[key].__setitem__(side, -1)
        fit = keys[-1]  # inner widths (lap5), widths (hdiff): W + E <= extent[0], S + N <= extent[1]
        yield f"{fit}-W+E=5", lambda s: s[fit].__setitem__(slice(0, 2), [2, 3])
        yield f"{fit}-S+N=5", lambda s: s[fit].__setitem__(slice(2, 4), [4, 1])
        yield f"{fit}-W+E=4-S+N=5", lambda s: s[fit].__setitem__(slice(0, 4), [2, 2, 0, 5])

    for tag, mutate in mutations():
        for also in ("", "+ax0=0", "+ax2=0", f"+{first}-null"):
            state = entry.base()
            mutate(state)
            if also.endswith("=0"):
                state["extent"][int(also[3])] = 0
            elif also:
                _break(entry, state, first)
            yield f"{entry.name}/widths/{tag}{also}", state
    if len(keys) == 2:  # lap5 ring: outer widths have no upper bound of their own, the fields must hold the grown domain
        state = entry.base()
        state["outer"] = [3, 1, 1, 1]
        yield f"{entry.name}/widths/outer[0]=3", state
        state = entry.base()
        state["outer"] = [1, 1, 1, 2]
        yield f"{entry.name}/widths/outer[3]=2", state
        # the overlap is looked for on the GROWN domain: `out` starts right behind inp's last row there, two rows further for the plain one
        state = entry.base()
        state["extent"][2] = 1
        state["out"][0]["ptr"] = state["inp"][0]["ptr"] + 6 * state["inp"][0]["strides"][1]
        yield f"{entry.name}/overlap/grown-domain-only", state


def cases():
    for entry in ENTRIES:
        for role, _, _ in entry.roles:
            yield from ((name, entry, state) for name, state in _field_cases(entry, role))
        gens = [_domain_cases(entry), _overlap_cases(entry)]
        if entry in LAP5 + LAP5_RING:
            gens.append(_variant_cases(entry))
        if entry in LAP5_RING:
            gens.append(_width_cases(entry, ("outer", "inner")))
        if entry in HDIFF_RING:
            gens.append(_width_cases(entry, ("widths",)))
        for gen in gens:
            yield from ((name, entry, state) for name, state in gen)


def _empty(state):
    return state["extent"] is not None and 0 in state["extent"]


def observe():
    """name -> [return code, message]; the message of an accepted call is not looked at."""
    out = {}
    lib = _lib.load()
    for name, entry, state in cases():
        assert name not in out, name
        rc = entry.run(copy.deepcopy(state))
        out[name] = [rc, lib.gt4mi_last_error().decode("ascii") if rc != 0 else ""]
    return out


def _guard(recorded):
    """Nothing in the table may reach a launch: a call that is not refused has an empty domain."""
    for name, _, state in cases():
        assert recorded[name][0] != 0 or _empty(state), f"{name} is accepted with a domain that is not empty: it would launch"


def test_nothing_in_the_table_can_launch():
    _guard(json.loads(GOLDEN.read_text())["cases"])


def test_the_table_reaches_every_refusal():
    golden = json.loads(GOLDEN.read_text())["cases"]
    for entry in ENTRIES:
        seen = {v[1] for k, v in golden.items() if k.startswith(entry.name + "/")}
        for role, _, _ in entry.roles:
            for needle in (f"field '{role}' is null", f"field '{role}': byte stride", f"field '{role}': origin", f"field '{role}': shape"):
                assert any(m.startswith(needle) for m in seen), (entry.name, needle)
        for needle in ("domain is null", "invalid domain size -1 along axis 2", "invalid domain size 2147483648 along axis 0"):
            assert needle in seen, (entry.name, needle)
        family = "lap5" if entry in LAP5 + LAP5_RING else "hdiff"
        overlaps = {m for m in seen if m.startswith(f"{family}: ") and "overlap in memory" in m and "coeff" not in m}
        assert len(overlaps) == 1, (entry.name, overlaps)
        assert ((LAP5_WHY in next(iter(overlaps))) == (entry in LAP5 + HDIFF)
                and (f"(see gt4mi_{family}_*)" in next(iter(overlaps))) == (entry in LAP5_RING + HDIFF_RING)), (entry.name, overlaps)
        if family == "lap5":
            assert {f"lap5: unknown variant {v}" for v in (-1, 4, 99)} <= seen, entry.name
        else:
            assert "hdiff: 'coeff' and 'out_field' overlap in memory without being the same elements" in seen, entry.name
        if entry in LAP5_RING:
            assert {"lap5 ring: null widths", "lap5 ring: negative width", "lap5 ring: inner widths do not fit the 4 x 4 domain"} <= seen
        if entry in HDIFF_RING:
            assert "hdiff ring: widths is null" in seen and sum(m.startswith("hdiff ring: widths (") for m in seen) >= 7, entry.name
        accepted = [k for k, v in golden.items() if k.startswith(entry.name + "/") and v[0] == 0]
        assert len(accepted) >= 7, (entry.name, accepted)  # (an empty domain along each axis, alone and with an overlap)


def test_every_refusal_is_what_the_fixture_recorded():
    golden = json.loads(GOLDEN.read_text())["cases"]
    _guard(golden)  # (before anything is called)
    have = observe()
    assert sorted(have) == sorted(golden)
    wrong = {name: (have[name], golden[name]) for name in golden if have[name] != golden[name]}
    assert not wrong, f"{len(wrong)} of {len(golden)} calls differ, the first: {next(iter(wrong.items()))}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_stencil_refusals.py --record")
    seen = observe()
    _guard(seen)
    lines = ",\n".join(f"{json.dumps(name)}: {json.dumps(value)}" for name, value in seen.items())  # one call per line
    GOLDEN.write_text(f'{{"cases": {{\n{lines}\n}}}}\n')
    print(f"recorded {len(seen)} calls in {GOLDEN}")
