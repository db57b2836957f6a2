"""The refusals of the eight multi-field utility entries (``gt4mi_halo_fill``, ``gt4mi_field_stats``, ``gt4mi_level_stats``,
``gt4mi_field_copy``, ``gt4mi_vertical_remap``, ``gt4mi_horizontal_interp``, ``gt4mi_horizontal_remap``, ``gt4mi_line_solve``), byte
for byte, without a GPU.

The entries share their per-field checks (csrc/field_args.hip.h); what a call is refused with -- return code and the bytes of
``gt4mi_last_error()`` -- and what an accepted call reports (``launches``, ``paths`` / ``path``, ``workspace_needed``) is behaviour, and
tests/golden/refusal_messages.json records it for a table of calls.  The table is generated: for every role of every entry
(dst, src, edge, position and coefficient fields, field and other) the same mutations of one base call -- null, misaligned, a stride that is
no multiple of the item size, stride 0 with an extent above 1 and of exactly 1, origins and shapes around every bound -- then
the overlaps, the buffers of the stats entries, the overlap tables of horizontal_remap, the axes, flags and workspace of
line_solve, and accepted calls of 1, 8 and 9 fields.  Every call carries made-up device addresses and the entry's dry-run flag, so
nothing is launched (the one exception: a stats or line_solve call WITHOUT its buffers is only refused when it is not a dry run;
the refusal is what keeps it from the GPU).

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
    pair = None      # (written role, read role) of an entry that takes pairs and refuses a written box that meets anything read

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
    pair = ("dst", "src")

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
    pair = ("dst", "src")

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
    pair = ("dst", "src")

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


TABLES = 0x6000000
TABLE_ARRAYS = ("ptr", "cell", "w", "h", "c", "den")


class HorizontalRemap(Entry):
    """extent stands for (nd_i, nd_j, nk); ns = nd + 1 unless nd == 1 (then 1), so that the two sides differ.  The six arrays of
    an axis are made-up device addresses like the fields: the host entry checks them and never reads through them.
    ``state["axis_i"]`` / ``["axis_j"]``: members that replace those of the axis the extent gives, or None for a null axis."""

    name = "horizontal_remap"
    roles = (("dst", True, ()), ("src", False, ()))
    nk = {"dst": 4, "src": 4}
    pair = ("dst", "src")

    def base(self, n=1):
        state = super().base(n)
        state.update(axis_i={}, axis_j={}, method=_lib.HREMAP_PLM, flags=_lib.HREMAP_DRY_RUN)
        return state

    def cells(self, state, ax):
        nd = state["extent"][ax]
        return (1 if nd == 1 else nd + 1), nd

    def box(self, state, role):
        ext = [self.cells(state, ax)[role == "dst"] for ax in (0, 1)] + [state["extent"][2]]
        return ext, [0, 0, 0], [0, 0, 0]

    def axis(self, state, ax):
        over = state["axis_" + "ij"[ax]]
        if over is None:
            return None
        ns, nd = self.cells(state, ax)
        members = {"ns": ns, "nd": nd, "nnz": ns + nd - 1}
        members.update({a: TABLES + ax * 0x100000 + n * 0x10000 for n, a in enumerate(TABLE_ARRAYS)})
        members.update(over)
        return ctypes.byref(_lib.OverlapAxis(**members))

    def run(self, s):
        launches = ctypes.c_int(77)
        rc = _lib.load().gt4mi_horizontal_remap(_table(s["dst"]), _table(s["src"]), s["n"], self.axis(s, 0), self.axis(s, 1),
                                                s["extent"][2], SIZE, s["method"], s["flags"], None, ctypes.byref(launches))
        return [rc, launches.value]


class LineSolve(Entry):
    """The base call solves along K (lanes along I); ``state["axis"]`` moves the line axis.  A run reports ``launches``,
    ``workspace_needed`` and ``path``."""

    name = "line_solve"
    roles = (("out", True, ()), ("rhs", False, ()), ("lower", False, (0, 1)), ("diag", False, (0, 1)), ("upper", False, (0, 1)))
    nk = {"out": 4, "rhs": 4, "lower": 4, "diag": 4, "upper": 4}
    pair = ("out", "rhs")

    def many(self, role):
        return role in ("out", "rhs")

    def base(self, n=1):
        state = super().base(n)
        state.update(axis=2, flags=_lib.LINE_DRY_RUN, workspace=WORK, workspace_bytes=1 << 20)
        return state

    def run(self, s):
        needed, path, launches = ctypes.c_int64(-5), ctypes.c_int(55), ctypes.c_int(77)
        rc = _lib.load().gt4mi_line_solve(_table(s["out"]), _table(s["rhs"]), s["n"], _one(s["lower"]), _one(s["diag"]), _one(s["upper"]),
                                          _i64(s["extent"]), s["axis"], SIZE, s["flags"], s["workspace"], s["workspace_bytes"], None,
                                          ctypes.byref(needed), ctypes.byref(path), ctypes.byref(launches))
        return [rc, launches.value, needed.value, path.value]


ENTRIES = (HaloFill(), Stats("field_stats"), Stats("level_stats"), FieldCopy(), VerticalRemap(), HorizontalInterp(), HorizontalRemap(),
           LineSolve())


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
    for entry in ENTRIES:
        if entry.pair is None:
            continue
        w, r = entry.pair  # the written and the read role: "dst" / "src", or "out" / "rhs"
        for a, b in (((w, 0), (r, 0)), ((w, 1), (r, 0)), ((w, 0), (r, 2)), ((w, 0), (w, 1)), ((w, 1), (w, 2)), ((w, 2), (r, 2))):
            for gap in (0, 8):  # the last byte of one box against the first of the other: touching, and one item apart
                state = entry.base(3)
                fa, fb = state[a[0]][a[1]], state[b[0]][b[1]]
                extent, lo, hi = entry.box(state, b[0])
                first = sum((fb["origin"][ax] - lo[ax]) * fb["strides"][ax] for ax in AXES)
                ext_a = entry.box(state, a[0])[0]
                last = sum((fa["origin"][ax] + ext_a[ax] - 1) * fa["strides"][ax] for ax in AXES)
                fb["ptr"] = fa["ptr"] + last - first + gap
                yield f"{entry.name}/overlap/{a[0]}{a[1]}-{b[0]}{b[1]}/gap={gap}", state
        for role, _, _ in entry.roles[2:]:  # edge, position and coefficient fields
            for k in (0, 2):
                state = entry.base(3)
                state[role][0]["ptr"] = state[w][k]["ptr"]
                yield f"{entry.name}/overlap/{w}{k}-{role}", state
            # two at once: the sweep goes dst by dst, and for one dst the shared fields come before the srcs (in line_solve out 0
            # on rhs 0 is an in-place pair and only the shared field is refused)
            for k in (0, 1):
                state = entry.base(3)
                state[r][0]["ptr"] = state[w][0]["ptr"]
                state[role][0]["ptr"] = state[w][k]["ptr"]
                yield f"{entry.name}/overlap/{w}0-{r}0+{w}{k}-{role}", state
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


def _origin_item(f):
    return f["ptr"] + sum(f["origin"][ax] * f["strides"][ax] for ax in AXES)


def _scalar_cases(entry):
    """The head checks that the generic generators cannot reach."""
    state = entry.base(2)
    state["n"] = 0
    yield f"{entry.name}/scalars/nfields=0", state
    state = entry.base(2)
    state["flags"] |= 2
    yield f"{entry.name}/scalars/unknown-flag", state
    for role in entry.pair:
        state = entry.base(2)
        state[role] = None
        yield f"{entry.name}/scalars/{role}-table-null", state


def _horizontal_remap_cases():
    entry = ENTRIES[6]

    def variant(name, n=2):
        return f"{entry.name}/tables/{name}", entry.base(n)

    yield from _scalar_cases(entry)
    for method in (_lib.HREMAP_PCM, _lib.HREMAP_PLM, 2):
        name, state = variant(f"method={method}")
        state["method"] = method
        yield name, state
    for nk in (0, -1, 1):
        name, state = variant(f"nk={nk}")
        state["extent"][2] = nk
        yield name, state
    for ax in "ij":
        key = "axis_" + ax
        name, state = variant(f"{key}-null")
        state[key] = None
        yield name, state
        ns, nd = entry.cells(state, 0)
        for member in ("ns", "nd"):
            for value in (0, -1):
                name, state = variant(f"{key}/{member}={value}")
                state[key] = {member: value, "nnz": 1}
                yield name, state
        for tag, nnz in (("nd-1", nd - 1), ("nd", nd), ("ns+nd-1", ns + nd - 1), ("ns+nd", ns + nd)):
            name, state = variant(f"{key}/nnz={tag}")
            state[key] = {"nnz": nnz}
            yield name, state
        # with pcm the kernel does not read h, c and den, and the entry must not look at them
        for mname, method in (("pcm", _lib.HREMAP_PCM), ("plm", _lib.HREMAP_PLM)):
            for n, array in enumerate(TABLE_ARRAYS):
                name, state = variant(f"{key}/{array}-null/{mname}")
                state["method"], state[key] = method, {array: 0}
                yield name, state
                name, state = variant(f"{key}/{array}-misaligned/{mname}")
                state["method"], state[key] = method, {array: TABLES + n * 0x10000 + (2 if n < 2 else 4)}
                yield name, state
                for k in (0, 2):  # a dst that meets a table array
                    name, state = variant(f"{key}/{array}-on-dst{k}/{mname}", 3)
                    state["method"], state[key] = method, {array: _origin_item(state["dst"][k])}
                    yield name, state
    # every array of one axis null at once: the first one is named
    name, state = variant("axis_j/all-null")
    state["axis_j"] = {array: 0 for array in TABLE_ARRAYS}
    yield name, state


def _line_solve_cases():
    entry = ENTRIES[7]

    def variant(name, n=2):
        return f"{entry.name}/{name}", entry.base(n)

    yield from _scalar_cases(entry)
    for role in ("lower", "diag", "upper"):
        name, state = variant(f"scalars/{role}-null")
        state[role] = None
        yield name, state
    for axis in (-1, 3):
        name, state = variant(f"scalars/axis={axis}")
        state["axis"] = axis
        yield name, state
    # in place: out[k] IS rhs[k], the same origin item and the same strides
    name, state = variant("inplace/every-pair")
    state["rhs"] = copy.deepcopy(state["out"])
    yield name, state
    name, state = variant("inplace/out0-is-rhs1")
    state["rhs"][1] = copy.deepcopy(state["out"][0])
    yield name, state
    name, state = variant("inplace/out0-on-rhs0-other-strides")  # the same origin item, I and J exchanged
    state["rhs"][0] = copy.deepcopy(state["out"][0])
    state["rhs"][0]["strides"] = [8 * SIZE, SIZE, 64 * SIZE]
    yield name, state
    name, state = variant("inplace/out0-on-rhs0-other-origin")  # the same strides, one item along
    state["rhs"][0] = copy.deepcopy(state["out"][0])
    state["rhs"][0]["origin"] = [3, 2, 0]
    yield name, state
    for axis in AXES:
        for periodic in (0, _lib.LINE_PERIODIC):
            tag = f"axis={axis}/periodic={periodic}"
            name, state = variant(f"accepted/{tag}")
            state["axis"], state["flags"] = axis, state["flags"] | periodic
            yield name, state
            for points in (0, 1, 2, 3):  # a periodic line needs 3 points; an empty box is accepted before that is asked
                name, state = variant(f"points={points}/{tag}")
                state["axis"], state["flags"] = axis, state["flags"] | periodic
                state["extent"][axis] = points
                yield name, state
    # one call per path, as field_copy/accepted/paths: the line axis with unit stride, another one, none
    name, state = variant("accepted/path=tiles")
    state["axis"] = 0
    yield name, state
    name, state = variant("accepted/path=lanes")
    yield name, state
    name, state = variant("accepted/path=lanes-along-k")  # K fastest, the lines along I: the lanes run along K
    for role, _, _ in entry.roles:
        for f in state[role]:
            f["strides"] = [4 * 8 * SIZE, 4 * SIZE, SIZE]
    state["axis"] = 0
    yield name, state
    name, state = variant("accepted/path=items")
    state["out"][1]["strides"] = [2 * SIZE, 16 * SIZE, 128 * SIZE]  # no unit stride
    state["out"][1]["ptr"] = 0x3000000
    yield name, state
    name, state = variant("accepted/path=tiles-1d-coefficients")  # a coefficient broadcast along the two other axes
    state["axis"] = 0
    for role in ("lower", "diag", "upper"):
        state[role][0]["strides"] = [SIZE, 0, 0]
    yield name, state
    # the workspace
    for periodic in (0, _lib.LINE_PERIODIC):
        tag = f"periodic={periodic}"
        name, state = variant(f"workspace/null-dry/{tag}")
        state["workspace"], state["flags"] = None, state["flags"] | periodic
        yield name, state
        # NOT a dry run, as in the stats entries the only such call: a missing workspace is refused only then, and the refusal is
        # all that keeps these made-up addresses from the device
        name, state = variant(f"workspace/null/{tag}")
        state["workspace"], state["flags"] = None, periodic
        yield name, state
        for short in (0, 8):
            name, state = variant(f"workspace/short-by-{short}/{tag}")
            state["flags"] |= periodic
            state["workspace_bytes"] = entry.run(copy.deepcopy(state))[2] - short
            yield name, state
    name, state = variant("workspace/misaligned")
    state["workspace"] += 4
    yield name, state
    for role, _, _ in entry.roles:
        for k in range(2 if entry.many(role) else 1):
            name, state = variant(f"workspace/overlaps-{role}{k}")
            state["workspace"] = _origin_item(state[role][k])
            yield name, state
            name, state = variant(f"workspace/ends-at-{role}{k}")  # its last byte is the one before the box
            state["workspace"] = _origin_item(state[role][k]) - entry.run(entry.base(2))[2]
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
    for gen in (_overlap_cases, _buffer_cases, _accepted_cases, _horizontal_remap_cases, _line_solve_cases):
        yield from ((name, by_name[name.split("/")[0]], state) for name, state in gen())


def observe():
    """name -> [return code, message, launches (, paths or workspace_needed (, path))]; the message of an accepted call is not looked at
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
    for name in ("field_copy", "vertical_remap", "horizontal_interp", "horizontal_remap"):
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
    for needle in ("axis_i is null", "axis_j is null", "axis_i has ns = 0 source", "axis_j has ns = 5 source and nd = -1 destination",
                   "axis_i has nnz = 3 terms", "axis_j has nnz = 9 terms", "nk = 0 levels", "unknown method 2", "unknown bits in flags",
                   "nfields = 0", *(f"axis_{ax} {array} is null" for ax in "ij" for array in TABLE_ARRAYS),
                   *(f"axis_{ax} {array} is not aligned to its item size" for ax in "ij" for array in TABLE_ARRAYS),
                   *(f"dst {k} and axis_{ax} {array} overlap" for k in (0, 2) for ax in "ij" for array in TABLE_ARRAYS)):
        assert any(m.startswith("horizontal_remap: ") and needle in m for m in seen), needle
    for needle in ("out 0 and rhs 0 overlap", "out 1 and rhs 0 overlap", "out 0 and rhs 2 overlap", "out 0 and out 1 overlap",
                   "out 1 and out 2 overlap", "out 0 and rhs 1 overlap", "out 0 and lower overlap", "out 2 and diag overlap",
                   "out 1 and upper overlap", "lower is null", "diag is null", "upper is null", "out is null", "rhs is null",
                   "axis -1 is not 0 (I), 1 (J) or 2 (K)", "axis 3 is not", "a periodic line needs at least 3 points, the extent along axis 0 is 2",
                   "the extent along axis 1 is 1", "the extent along axis 2 is 2", "workspace is null", "is too small", "nfields = 0",
                   "unknown bits in flags", "workspace is not aligned to 8 bytes", "workspace overlaps out 1", "workspace overlaps rhs 0",
                   "workspace overlaps lower", "workspace overlaps diag", "workspace overlaps upper"):
        assert any(m.startswith("line_solve: ") and needle in m for m in seen), needle
    # what accepted line_solve calls report: every path, and a periodic workspace twice the plain one
    cases = json.loads(GOLDEN.read_text())["cases"]
    assert {cases[f"line_solve/accepted/path={p}"][-1] for p in ("lanes", "tiles", "items")} == \
        {_lib.LINE_PATH_LANES, _lib.LINE_PATH_TILES, _lib.LINE_PATH_ITEMS}
    for axis in AXES:
        plain, periodic = (cases[f"line_solve/accepted/axis={axis}/periodic={p}"] for p in (0, _lib.LINE_PERIODIC))
        assert plain[0] == periodic[0] == 0 and plain[3] > 0 and periodic[3] == 2 * plain[3]
    for array in ("h", "c", "den"):  # pcm does not look at them
        for what in ("null", "misaligned", "on-dst0"):
            assert cases[f"horizontal_remap/tables/axis_i/{array}-{what}/pcm"][0] == 0


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
