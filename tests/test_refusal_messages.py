"""The refusals of the six multi-field utility entries (``gt4mi_halo_fill``, ``gt4mi_field_stats``, ``gt4mi_level_stats``,
``gt4mi_field_copy``, ``gt4mi_vertical_remap``, ``gt4mi_horizontal_interp``), byte for byte, without a GPU.

The entries share their per-field checks (csrc/field_args.hip.h); what a call is refused with -- return code and the bytes of
``gt4mi_last_error()`` -- and what an accepted call reports (``launches``, ``paths``, ``workspace_needed``) is behaviour, and
tests/golden/refusal_messages.json records it for a table of calls.  The table is generated: for every role of every entry
(dst, src, edge and position fields, field and other) the same mutations of one base call -- null, misaligned, a stride that is
no multiple of the item size, stride 0 with an extent above 1 and of exactly 1, origins and shapes around every bound -- then
the overlaps, the buffers of the stats entries, and accepted calls of 1, 8 and 9 fields.  Every call carries made-up device
addresses and the entry's dry-run flag, so nothing is launched (the one exception: a stats call WITHOUT its buffers is only
refused when it is not a dry run; the refusal is what keeps it from the GPU).

The fixture is recorded from a build of the commit BEFORE a change to the checks, never from the code under test:

    python tests/test_refusal_messages.py --record      # in a tree of the parent commit, after build()

Cases named in ``hand_edited`` of the fixture were changed by hand afterwards, with the reason next to them."""

import copy
import ctypes
import json
import pathlib
import sys

if __name__ == "__main__":
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

from gt4py_amd import _lib

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "refusal_messages.json"
SIZE = 8
WORK, RESULT = 0x4000000, 0x5000000
AXES = range(3)


def _spec(ptr, nk):
    """One field of shape (8, 8, nk), I-contiguous, origin (2, 2, 0)."""
    return {"ptr": ptr, "shape": [8, 8, nk], "strides": [SIZE, 8 * SIZE, 64 * SIZE], "origin": [2, 2, 0]}


def _table(specs):
    if specs is None:
        return None
    out = (_lib.Field * max(len(specs), 1))()
    for n, s in enumerate(specs):
        out[n] = _lib.Field.make(s["ptr"], s["shape"], s["strides"], s["origin"])
    return out


def _one(specs):
    return None if specs is None else ctypes.byref(_table(specs)[0])


def _i64(values):
    return None if values is None else (ctypes.c_int64 * len(values))(*values)


class Entry:
    """One C entry: ``base(n)`` is an accepted call of ``n`` fields (a dict: role -> list of field specs, plus scalars), ``run``
    makes the call, ``box`` says which box of a role's fields the call touches (extent, reach below, reach above)."""

    name = ""
    roles = ()       # (role, written, axes that may be broadcast)
    nk = {}          # role -> levels of its fields

    def base(self, n=1):
        state = {role: [_spec((r + 1) * 0x100000 + k * 0x2000, self.nk[role]) for k in range(n if self.many(role) else 1)]
                 for r, (role, _, _) in enumerate(self.roles)}
        state["n"] = n
        state["extent"] = [4, 4, 4]
        return state

    def many(self, role):
        return True

    def box(self, state, role):
        return list(state["extent"]), [0, 0, 0], [0, 0, 0]

    def shrink(self, state, ax):
        """The same call with an extent of exactly 1 along ``ax``."""
        state["extent"][ax] = 1


class HaloFill(Entry):
    name = "halo_fill"
    roles = (("field", True, ()),)
    nk = {"field": 4}

    def base(self, n=1):
        state = super().base(n)
        state["halo"] = [1, 1, 1, 1]
        return state

    def box(self, state, role):
        h = state["halo"]
        return list(state["extent"]), [h[0], h[2], 0], [h[1], h[3], 0]

    def run(self, s):
        launches = ctypes.c_int(77)
        rc = _lib.load().gt4mi_halo_fill(_table(s["field"]), s["n"], _i64(s["extent"]), _i64(s["halo"]), _lib.HALO_ZERO_GRADIENT,
                                         _lib.HALO_ZERO_GRADIENT, _lib.HALO_ALL_SIDES | _lib.HALO_DRY_RUN, b"\0" * 8, SIZE, None,
                                         ctypes.byref(launches))
        return [rc, launches.value]


class Stats(Entry):
    roles = (("field", False, ()), ("other", False, (0, 1, 2)))
    nk = {"field": 4, "other": 4}

    def __init__(self, name):
        self.name = name

    def base(self, n=1):
        state = super().base(n)
        state.update(workspace=WORK, workspace_bytes=1 << 20, result=RESULT, flags=_lib.STATS_DRY_RUN)
        return state

    def run(self, s):
        needed, launches = ctypes.c_int64(-5), ctypes.c_int(77)
        rc = getattr(_lib.load(), "gt4mi_" + self.name)(_table(s["field"]), _table(s["other"]), s["n"], _i64(s["extent"]), SIZE,
                                                        s["workspace"], s["workspace_bytes"], s["result"], s["flags"], None,
                                                        ctypes.byref(needed), ctypes.byref(launches))
        return [rc, launches.value, needed.value]


class FieldCopy(Entry):
    name = "field_copy"
    roles = (("dst", True, ()), ("src", False, ()))
    nk = {"dst": 4, "src": 4}

    def run(self, s):
        launches = ctypes.c_int(77)
        paths = (ctypes.c_int * max(s["n"], 1))(*([-1] * max(s["n"], 1)))
        rc = _lib.load().gt4mi_field_copy(_table(s["dst"]), _table(s["src"]), s["n"], _i64(s["extent"]), SIZE, SIZE, _lib.COPY_DRY_RUN,
                                          None, paths, ctypes.byref(launches))
        return [rc, launches.value, list(paths)]


class VerticalRemap(Entry):
    """extent[2] stands for nd; ns = nd + 1 unless nd == 1 (then 1), so that the two sides differ."""

    name = "vertical_remap"
    roles = (("dst", True, ()), ("src", False, ()), ("src_edges", False, (0, 1)), ("dst_edges", False, (0, 1)))
    nk = {"dst": 6, "src": 6, "src_edges": 6, "dst_edges": 6}

    def many(self, role):
        return role in ("dst", "src")

    def levels(self, state):
        nd = state["extent"][2]
        return (1 if nd == 1 else nd + 1), nd

    def box(self, state, role):
        ns, nd = self.levels(state)
        nk = {"dst": nd, "src": ns, "src_edges": ns + 1, "dst_edges": nd + 1}[role]
        return [state["extent"][0], state["extent"][1], nk], [0, 0, 0], [0, 0, 0]

    def run(self, s):
        launches = ctypes.c_int(77)
        ns, nd = self.levels(s)
        rc = _lib.load().gt4mi_vertical_remap(_table(s["dst"]), _table(s["src"]), s["n"], _one(s["src_edges"]), _one(s["dst_edges"]),
                                              _i64(s["extent"][:2]), ns, nd, SIZE, SIZE, _lib.REMAP_PLM, _lib.REMAP_DRY_RUN, None,
                                              ctypes.byref(launches))
        return [rc, launches.value]


class HorizontalInterp(Entry):
    name = "horizontal_interp"
    roles = (("dst", True, ()), ("src", False, ()), ("pos_i", False, (2,)), ("pos_j", False, (2,)))
    nk = {"dst": 4, "src": 4, "pos_i": 4, "pos_j": 4}

    def many(self, role):
        return role in ("dst", "src")

    def base(self, n=1):
        state = super().base(n)
        state["reach"] = [1, 2, 2, 1]
        return state

    def box(self, state, role):
        r = state["reach"] if role == "src" else [0, 0, 0, 0]
        return list(state["extent"]), [r[0], r[2], 0], [r[1], r[3], 0]

    def run(self, s):
        launches = ctypes.c_int(77)
        rc = _lib.load().gt4mi_horizontal_interp(_table(s["dst"]), _table(s["src"]), s["n"], _one(s["pos_i"]), _one(s["pos_j"]),
                                                 _i64(s["extent"]), _i64(s["reach"]), SIZE, SIZE, _lib.INTERP_CUBIC,
                                                 _lib.INTERP_DRY_RUN, None, ctypes.byref(launches))
        return [rc, launches.value]


ENTRIES = (HaloFill(), Stats("field_stats"), Stats("level_stats"), FieldCopy(), VerticalRemap(), HorizontalInterp())


def _field_cases(entry, role):
    """(name, state) for every mutation of the first and of the last field of ``role`` in a call of two fields."""
    def variant(name, ext1=None):
        state = entry.base(2)
        if ext1 is not None:
            entry.shrink(state, ext1)
        k = len(state[role]) - 1
        return f"{entry.name}/{role}{k}/{name}", state, state[role][k]

    name, state, f = variant("null")
    f["ptr"] = 0
    yield name, state
    name, state, f = variant("misaligned")
    f["ptr"] += 4
    yield name, state
    for ax in AXES:
        name, state, f = variant(f"stride{ax}+4")
        f["strides"][ax] += 4
        yield name, state
        # stride 0 (s0) or not, the extent along the axis as in the base call or exactly 1 (e1), and around every bound:
        # the origin at -1, one below the reach and at the reach; the shape one short of what the box needs and just enough
        for zero in (False, True):
            for ext1 in (None, ax) if zero else (None,):
                tag = f"ax{ax}" + ("/s0" if zero else "") + ("/e1" if ext1 is not None else "")
                _, state, _ = variant("", ext1)
                extent, lo, hi = entry.box(state, role)
                for origin in sorted({-1, lo[ax] - 1, lo[ax], 2}):
                    for short in (1, 0, None):
                        name, state, f = variant(f"{tag}/origin={origin}/shape={'base' if short is None else f'need-{short}'}", ext1)
                        if zero:
                            f["strides"][ax] = 0
                        f["origin"][ax] = origin
                        if short is not None:
                            f["shape"][ax] = origin + extent[ax] + hi[ax] - short
                        yield name, state


def _overlap_cases():
    for entry in ENTRIES[3:]:
        for a, b in (("dst0", "src0"), ("dst1", "src0"), ("dst0", "src2"), ("dst0", "dst1"), ("dst1", "dst2"), ("dst2", "src2")):
            for gap in (0, 8):  # the last byte of one box against the first of the other: touching, and one item apart
                state = entry.base(3)
                fa, fb = state[a[:3]][int(a[3])], state[b[:3]][int(b[3])]
                extent, lo, hi = entry.box(state, b[:3])
                first = sum((fb["origin"][ax] - lo[ax]) * fb["strides"][ax] for ax in AXES)
                ext_a = entry.box(state, a[:3])[0]
                last = sum((fa["origin"][ax] + ext_a[ax] - 1) * fa["strides"][ax] for ax in AXES)
                fb["ptr"] = fa["ptr"] + last - first + gap
                yield f"{entry.name}/overlap/{a}-{b}/gap={gap}", state
        for role, _, _ in entry.roles[2:]:  # edge and position fields
            for k in (0, 2):
                state = entry.base(3)
                state[role][0]["ptr"] = state["dst"][k]["ptr"]
                yield f"{entry.name}/overlap/dst{k}-{role}", state
            # two at once: the sweep goes dst by dst, and for one dst the shared fields come before the srcs
            for k in (0, 1):
                state = entry.base(3)
                state["src"][0]["ptr"] = state["dst"][0]["ptr"]
                state[role][0]["ptr"] = state["dst"][k]["ptr"]
                yield f"{entry.name}/overlap/dst0-src0+dst{k}-{role}", state
    # the reach of a src alone makes it meet a dst: the dst ends one row below src's box
    entry = ENTRIES[5]
    for reach in ([1, 2, 2, 1], [1, 2, 0, 1]):
        state = entry.base(1)
        state["reach"] = reach
        d, s = state["dst"][0], state["src"][0]
        s["ptr"] = d["ptr"] + (d["origin"][1] + 4) * 64 - s["origin"][1] * 64 + 64
        s["shape"][2] = d["shape"][2] = 1
        state["extent"][2] = 1
        yield f"{entry.name}/overlap/reach={reach[2]}", state


def _buffer_cases():
    for entry in ENTRIES[1:3]:
        def variant(name, n=2):
            state = entry.base(n)
            return f"{entry.name}/buffers/{name}", state

        for which in ("workspace", "result"):
            name, state = variant(f"{which}-null-dry")
            state[which] = None
            yield name, state
            # NOT a dry run, the only such call of the table: a missing buffer is refused only then.  The refusal is all that
            # keeps these made-up addresses from the device, so in the entries it stays in front of everything that launches
            # (tests/test_diagnostics.py and tests/test_level_stats.py provoke their refusals the same way)
            name, state = variant(f"{which}-null")
            state[which], state["flags"] = None, 0
            yield name, state
            name, state = variant(f"{which}-misaligned")
            state[which] += 4
            yield name, state
            for role in ("field", "other"):
                for k in (0, 1):
                    name, state = variant(f"{which}-overlaps-{role}{k}")
                    f = state[role][k]
                    state[which] = f["ptr"] + sum(f["origin"][ax] * f["strides"][ax] for ax in AXES)
                    yield name, state
                    name, state = variant(f"{which}-ends-at-{role}{k}")
                    f = state[role][k]
                    state[which] = f["ptr"] + sum((f["origin"][ax] + 3) * f["strides"][ax] for ax in AXES) + SIZE
                    yield name, state
        name, state = variant("both-null-dry")
        state["workspace"] = state["result"] = None
        yield name, state
        for short in (0, 8):
            name, state = variant(f"workspace-short-by-{short}")
            probe = entry.base(2)
            state["workspace_bytes"] = entry.run(probe)[2] - short
            yield name, state
        name, state = variant("workspace-overlaps-result")
        state["result"] = state["workspace"] + 64
        yield name, state
        name, state = variant("result-overlaps-workspace")
        state["workspace"] = state["result"] + 8
        yield name, state
        # an absent second field: data == NULL is "no other", whatever else the descriptor holds
        name, state = variant("other1-absent")
        state["other"][1].update(ptr=0, strides=[3, 3, 3], origin=[-1, -1, -1])
        yield name, state
        name, state = variant("others-null")
        state["other"] = None
        yield name, state


def _accepted_cases():
    for entry in ENTRIES:
        for n in (1, 8, 9):
            yield f"{entry.name}/accepted/n={n}", entry.base(n)
    # field_copy: one pair of every path in one call
    entry = ENTRIES[3]
    state = entry.base(3)
    state["dst"][1]["strides"] = [4 * 8 * SIZE, 4 * SIZE, SIZE]   # K fastest: tiles
    state["dst"][2]["strides"] = [2 * SIZE, 16 * SIZE, 128 * SIZE]  # no unit stride: items
    state["dst"][2]["ptr"] = 0x3000000
    yield "field_copy/accepted/paths", state


def cases():
    for entry in ENTRIES:
        for role, _, _ in entry.roles:
            yield from ((name, entry, state) for name, state in _field_cases(entry, role))
    by_name = {e.name: e for e in ENTRIES}
    for gen in (_overlap_cases, _buffer_cases, _accepted_cases):
        yield from ((name, by_name[name.split("/")[0]], state) for name, state in gen())


def observe():
    """name -> [return code, message, launches (, paths or workspace_needed)]; the message of an accepted call is not looked at
    (``gt4mi_last_error`` keeps the last refusal)."""
    out = {}
    lib = _lib.load()
    for name, entry, state in cases():
        assert name not in out, name
        rc, *rest = entry.run(copy.deepcopy(state))
        out[name] = [rc, lib.gt4mi_last_error().decode("ascii") if rc != 0 else "", *rest]
    return out


def test_the_table_reaches_every_branch():
    """Every message of the per-field check, of the sweeps and of the buffer checks occurs, for every role it can occur for."""
    seen = {v[1] for v in json.loads(GOLDEN.read_text())["cases"].values()}
    for entry in ENTRIES[1:]:
        for role, written, broadcast in entry.roles:
            who = f"{entry.name}: {role} "
            needles = ["is not aligned to its item size", "is not a multiple of the item size", "negative origin", "is outside the array"]
            if role != "other":
                needles.append("is null")
            for needle in needles:
                assert any(m.startswith(who) and needle in m for m in seen), (who, needle)
            if written or role == "field":
                assert any(m.startswith(who) and "has stride 0 along axis" in m for m in seen), who
    for name in ("field_copy", "vertical_remap", "horizontal_interp"):
        for needle in ("dst 0 and src 0 overlap", "dst 1 and src 0 overlap", "dst 0 and src 2 overlap", "dst 0 and dst 1 overlap",
                       "dst 1 and dst 2 overlap"):
            assert any(m.startswith(name) and needle in m for m in seen), (name, needle)
    for needle in ("dst 0 and src_edges overlap", "dst 2 and dst_edges overlap", "dst 0 and pos_i overlap", "dst 2 and pos_j overlap",
                   "leaves no room for a reach", "+ reach 2 along axis 0"):
        assert any(needle in m for m in seen), needle
    for name in ("field_stats", "level_stats"):
        for needle in ("workspace is null", "result is null", "is too small", "workspace is not aligned", "result is not aligned",
                       "workspace overlaps field 1", "result overlaps other 0", "workspace overlaps result"):
            assert any(m.startswith(name) and needle in m for m in seen), (name, needle)


def test_every_refusal_and_every_accepted_call_is_what_the_fixture_recorded():
    golden = json.loads(GOLDEN.read_text())["cases"]
    have = observe()
    assert sorted(have) == sorted(golden)
    wrong = {name: (have[name], golden[name]) for name in golden if have[name] != golden[name]}
    assert not wrong, f"{len(wrong)} of {len(golden)} calls differ, the first: {next(iter(wrong.items()))}"
    refused = sum(1 for v in golden.values() if v[0] != 0)
    assert refused > 300 and len(golden) - refused > 100  # (the table holds both kinds)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_refusal_messages.py --record")
    old = json.loads(GOLDEN.read_text()) if GOLDEN.exists() else {}
    seen = observe()
    lines = ",\n".join(f"{json.dumps(name)}: {json.dumps(value)}" for name, value in seen.items())  # one call per line
    GOLDEN.write_text(f'{{"hand_edited": {json.dumps(old.get("hand_edited", {}))},\n"cases": {{\n{lines}\n}}}}\n')
    print(f"recorded {len(seen)} calls in {GOLDEN}")
