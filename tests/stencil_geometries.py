"""A catalogue of storage geometries for the arguments of a generated stencil, each there to turn one condition of the generic
executor's choice of kernel twin, and the byte-for-byte comparison of what a call leaves in them.

Built on ``device_layouts``: every field lives in a FLAT buffer of integers that holds a sentinel everywhere except the field's
view, reaches one ghost row and one ghost column beyond what the product is handed, and is compared whole after the call.  Handled
fully: fields that have all of I, J, K and no data dimension.  Lower-dimensional fields and fields with data dimensions keep
the storage the other fuzz tests give them (``gt_storage.from_array`` with the aligned index on the origin, whatever the geometry:
a program that has such a field with an I axis therefore has no common lead in `lead1` .. `lead3`); they are listed in
``Case.plain`` and compared through ``get()``.  Negative strides are not covered.

Test infrastructure; imports no product code and (at import) no torch."""

from __future__ import annotations

import numpy as np

import device_layouts as L

GEOMETRIES = {
    "preset": "control: I-contiguous, padded rows, every origin on its aligned column -- lead 0, lane twins eligible",
    "lead1": "every origin 1 item past its aligned column: a common lead of 1 (strips start before the domain)",
    "lead2": "every origin 2 items past its aligned column: lead 2 in 4-byte fields, 0 in 8-byte ones",
    "lead3": "every origin 3 items past its aligned column: lead 3 in 4-byte fields, 1 in 8-byte ones",
    "mixed_lead": "one written field 1 item off, the others aligned: the common lead is 0, that field's origin fails the lane test",
    "odd_pitch": "an odd J pitch (and K stride): pitch modulo the lane width is not 0",
    "odd_plane": "aligned origin and pitch, K stride one item longer than pitch * nj: only the K stride fails the lane test",
    "kfirst": "K-contiguous (C order): I stride is not 1",
    "jfirst": "J-contiguous: I stride is not 1",
    "sub_box": "preset buffers, the compute box 5 columns and 2 rows inside live data: lead 5 modulo the lane width",
    "j_halves": "two fields as the low and high rows of one I-contiguous parent: overlapping spans, no common element, unit I stride",
    "interleaved": "two fields as parent[..., 0] and parent[..., 1]: overlapping spans, no common element, I stride 2",
}
ALIAS = ("j_halves", "interleaved")
#: the variant key (unit I stride, no alias) each geometry is there to select
VARIANT = {g: (g not in ("kfirst", "jfirst", "interleaved"), g not in ALIAS) for g in GEOMETRIES}
#: the smallest domains that reach the seams: less than one wave of lanes; across the 124-column (8-byte) and 248-column (4-byte)
#: wave seam of the `_vecs` strips and two waves of `_vec`
DOMAINS = [(37, 11, 3), (253, 6, 2)]
SUB_BOX_SHIFT, SUB_BOX_SHRINK = (5, 2, 0), (6, 3, 0)


class LeftOut(Exception):
    """The geometry does not apply to this program (the reason is the message)."""


def lane(itemsize: int) -> int:
    """Items of a 16-byte lane."""
    return max(16 // itemsize, 1)


def is_full(info) -> bool:
    return tuple(info.axes) == ("I", "J", "K") and not tuple(info.data_dims)


def _odd_plane(shape, itemsize, align_i):
    numel, (si, pitch, _), offset = L.geometry(shape, "ifirst", itemsize, align_i)
    sk = pitch * shape[1] + 1
    return sk * shape[2] + 2 * (256 // itemsize), (si, pitch, sk), offset


def _pair(full, written, itemsize):
    """The two fields an alias geometry puts into one parent: the first written one that has a partner of its item size, and that
    partner (a read-only one where there is one)."""
    for w in full:
        if w not in written:
            continue
        same = [x for x in full if x != w and itemsize[x] == itemsize[w]]
        if same:
            return w, next((x for x in same if x not in written), same[0])
    raise LeftOut("no two I-J-K fields of equal item size with one of them written")


class Case:
    """The placement of the arguments of one call in one geometry.

    ``arrays`` / ``origins``: as ``stencil_zoo.make_inputs`` gives them; ``field_info``: the stencil's; ``written``: the names the
    program assigns, ``used``: those it reads or assigns (default: all; an argument the program never touches makes no alias).
    ``buffers``: {buffer: (items, item size)}; ``fields``: {name: (buffer, shape, strides in items)} of the fully
    handled fields, ``plain``: {name: aligned index} of the others; ``origins`` and ``domain``: what the call is made with."""

    def __init__(self, geometry, arrays, origins, field_info, written, domain, region_reach=0, used=None):
        if geometry not in GEOMETRIES:
            raise ValueError(geometry)
        self.geometry, self.written = geometry, frozenset(written)
        self.dtype = {k: v.dtype for k, v in arrays.items()}
        self.shape = {k: tuple(v.shape) for k, v in arrays.items()}
        full = [k for k in arrays if is_full(field_info[k])]
        self.origins, self.domain = dict(origins), tuple(domain)
        shift = {"lead1": 1, "lead2": 2, "lead3": 3}.get(geometry, 0)
        self.off_column = None
        if geometry == "mixed_lead":
            lanes = [k for k in full if k in self.written and self.dtype[k].itemsize in (4, 8)]
            self.off_column = (lanes or [k for k in full if k in self.written] or full)[0]
        if geometry == "sub_box":
            self.domain = tuple(d - s for d, s in zip(domain, SUB_BOX_SHRINK))
            if min(self.domain[:2]) < max(region_reach, 1):
                raise LeftOut("a horizontal region wider than the shrunk domain")
            for k, info in field_info.items():
                if k in arrays:
                    move = dict(zip("IJK", SUB_BOX_SHIFT))
                    self.origins[k] = tuple(o + move[a] for o, a in zip(origins[k], info.axes)) + tuple(origins[k][len(info.axes):])
        touched = [k for k in full if used is None or k in used]
        self.pair = _pair(touched, self.written, {k: self.dtype[k].itemsize for k in full}) if geometry in ALIAS else ()
        self.plain = {}
        for k in arrays:
            if k not in full:
                self.plain[k] = tuple(origins[k])
        self.buffers, self.fields, self._offset = {}, {}, {}
        for k in full:
            if k in self.pair:
                continue
            isz, ext = self.dtype[k].itemsize, self._ext(k)
            align = origins[k][0] - shift - (1 if k == self.off_column else 0)
            if geometry in ("kfirst", "jfirst"):
                numel, strides, offset = L.geometry(ext, geometry, isz, 0)
            elif geometry == "odd_pitch":
                numel, strides, offset = L.geometry(ext, "ifirst_unaligned", isz, 0)
            elif geometry == "odd_plane":
                numel, strides, offset = _odd_plane(ext, isz, align)
            else:
                numel, strides, offset = L.geometry(ext, "ifirst", isz, align)
            self.buffers[k] = (numel, isz)
            self.fields[k] = (k, self.shape[k], strides)
            self._offset[k] = offset
        if self.pair:
            self._place_pair(origins)
        self.offset = {}

    def _ext(self, k):
        ni, nj, nk = self.shape[k]
        return (ni + 1, nj + 1, nk)

    def _place_pair(self, origins):
        a, b = self.pair
        isz = self.dtype[a].itemsize
        items = 256 // isz
        (nia, nja, nka), (nib, njb, nkb) = self._ext(a), self._ext(b)
        nk = max(nka, nkb)
        if self.geometry == "j_halves":  # both origins on a 256-byte boundary, every row inside its own pitch
            lead = {k: (items - origins[k][0] % items) % items for k in (a, b)}
            pitch = -(-max(lead[a] + nia, lead[b] + nib) // items) * items
            strides = (1, pitch, pitch * (nja + njb))
            start = {a: lead[a], b: pitch * nja + lead[b]}
            numel = strides[2] * nk + 2 * items
        else:
            pitch = -(-max(nia, nib) // items) * items
            strides = (2, 2 * pitch, 2 * pitch * max(nja, njb))
            start = {a: 0, b: 1}
            numel = strides[2] * nk + 2 * items
        self.buffers["pair"] = (numel, isz)
        for k in (a, b):
            self.fields[k] = ("pair", self.shape[k], strides)
            self._offset[k] = lambda ptr, s=start[k]: (-(ptr // isz)) % items + s

    # ---- the flat images ------------------------------------------------------------------------------------------------------
    def resolve(self, ptr_of):
        """Fix the offsets (items from the start of the flat buffer) for buffers at the addresses ``ptr_of``: {buffer: address}."""
        self.offset = {k: self._offset[k](ptr_of[buf]) for k, (buf, _, _) in self.fields.items()}
        return self

    def view(self, images, k, ghosts=False):
        """Field ``k`` in the host images, as integers: what the product is handed, or with the ghost row and column."""
        buf, shape, strides = self.fields[k]
        return L.host_view(images[buf], self._ext(k) if ghosts else shape, strides, self.offset[k])

    def _store(self, k):
        """The integer type the flat buffer of field ``k`` is kept in."""
        return L.NP_INT[self.dtype[k].itemsize]

    def images(self, arrays):
        """{buffer: flat host image}: the sentinel everywhere, ``arrays[k]`` in the view of every field."""
        out = {buf: L.sentinel_image(numel, isz) for buf, (numel, isz) in self.buffers.items()}
        for k in self.fields:
            self.view(out, k)[...] = arrays[k].view(self._store(k))
        return out

    def host_views(self, images):
        """{name: the strided host view, in the field's dtype} of the fully handled fields."""
        return {k: self.view(images, k).view(self.dtype[k]) for k in self.fields}

    def origin_pointer(self, ptr_of, k):
        buf, _, strides = self.fields[k]
        return ptr_of[buf] + (self.offset[k] + sum(o * s for o, s in zip(self.origins[k], strides))) * self.dtype[k].itemsize

    def span(self, ptr_of, k):
        """[first byte, last byte + 1) of what the product is handed."""
        buf, shape, strides = self.fields[k]
        isz = self.dtype[k].itemsize
        lo = ptr_of[buf] + self.offset[k] * isz
        return lo, lo + (sum((n - 1) * s for n, s in zip(shape, strides)) + 1) * isz

    # ---- the comparison -------------------------------------------------------------------------------------------------------
    def compare(self, before, expect, got, what=""):
        """``got``: the flat buffers after the call; ``before``: the images they held; ``expect``: {name: the oracle's whole
        array}.  Every item of every buffer must equal, as an integer, the image with the oracle's arrays in the views; inside the
        view of a field the program writes a NaN matches a NaN of any payload (the sign of a zero counts everywhere).  The buffer
        of a field the program does not write must be unchanged in every byte."""
        want = {buf: image.copy() for buf, image in before.items()}
        for k in self.fields:
            if k in self.written:
                self.view(want, k)[...] = expect[k].view(self._store(k))
            else:
                assert np.array_equal(expect[k].view(self._store(k)), self.view(before, k)), f"{what}: the reference changed the input {k}"
        for buf in self.buffers:
            members = [k for k in self.fields if self.fields[k][0] == buf]
            ok = got[buf] == want[buf]
            inside = np.zeros(want[buf].shape, dtype=bool)
            for k in members:
                mine = np.zeros(want[buf].shape, dtype=bool)
                L.host_view(mine, self.fields[k][1], self.fields[k][2], self.offset[k])[...] = True
                inside |= mine
                if k in self.written and self.dtype[k].kind == "f":
                    ok |= mine & np.isnan(got[buf].view(self.dtype[k])) & np.isnan(want[buf].view(self.dtype[k]))
            if not ok.all():
                bad = np.flatnonzero(~ok)
                where = "; ".join(f"{k}{'' if k in self.written else ' (not written)'}: offset {self.offset[k]}, strides {self.fields[k][2]}, "
                                  f"shape {self.fields[k][1]}, origin {self.origins[k]}" for k in members)
                raise AssertionError(f"{what}: buffer of {', '.join(members)}: {bad.size} items of the whole buffer differ "
                                     f"({int((~ok & inside).sum())} of them in a view), first at flat index {bad[:8].tolist()} ({where}); "
                                     f"got {got[buf][bad[:8]].tolist()}, want {want[buf][bad[:8]].tolist()}")


class DeviceCase:
    """The device side of a ``Case``: the flat buffers on the GPU, the images they were filled with, and the strided views."""

    def __init__(self, case: Case, arrays):
        import torch

        flat_t = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
        view_t = {"bool": torch.bool, "int8": torch.int8, "int16": torch.int16, "int32": torch.int32, "int64": torch.int64,
                  "float32": torch.float32, "float64": torch.float64}
        self.case = case
        self.flat = {buf: torch.empty(numel, dtype=flat_t[isz], device="cuda") for buf, (numel, isz) in case.buffers.items()}
        self.ptr_of = {buf: t.data_ptr() for buf, t in self.flat.items()}
        case.resolve(self.ptr_of)
        self.before = case.images(arrays)
        for buf, t in self.flat.items():
            t.copy_(torch.from_numpy(self.before[buf]))
        self.views = {k: torch.as_strided(self.flat[buf].view(view_t[case.dtype[k].name]), shape, strides, case.offset[k])
                      for k, (buf, shape, strides) in case.fields.items()}

    def download(self):
        return {buf: t.cpu().numpy() for buf, t in self.flat.items()}
