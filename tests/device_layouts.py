"""The four memory layouts the GPU tests put their arrays in, for items of 1, 2, 4 and 8 bytes: the geometry (torch-free, so that
the CPU tests can check it), device buffers kept FLAT so that every byte of them can be compared, and the sentinel those bytes hold.
Test infrastructure; imports no product code and (at import) no torch."""

from __future__ import annotations

import numpy as np

LAYOUTS = ["ifirst", "ifirst_unaligned", "kfirst", "jfirst"]
DOMAINS = [(1, 1, 1), (3, 5, 2), (17, 33, 5), (64, 64, 8), (65, 63, 7), (130, 40, 3), (300, 37, 2)]
#: 1-byte: a bit pattern; 2-byte: float16's NaN with a payload; 4, 8: NaNs with a payload no arithmetic produces
SENTINEL = {1: 0xA5, 2: 0x7DAD, 4: 0x7FA0_BEEF, 8: 0x7FF4_DEAD_BEEF_0001}
NP_INT = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}  # (what torch has)
NP_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def geometry(shape, layout: str, itemsize: int, align_i: int):
    """(items of the flat buffer, strides in items, offset(address of the flat buffer) in items) of a layout."""
    ni, nj, nk = shape
    if layout == "ifirst":  # rows padded to 256 bytes, the column `align_i` on a 256-byte boundary
        items = 256 // itemsize
        pitch = -(-ni // items) * items
        lead = (items - align_i % items) % items
        return pitch * nj * nk + 2 * items, (1, pitch, pitch * nj), lambda ptr: (-(ptr // itemsize) % items + lead) % items
    if layout == "ifirst_unaligned":  # an odd pitch, the first item on an odd item address
        pitch = ni + 3 if (ni + 3) % 2 else ni + 4
        return pitch * nj * nk + 8, (1, pitch, pitch * nj), lambda ptr: 1 if (ptr // itemsize) % 2 == 0 else 2
    if layout == "kfirst":  # numpy's C order
        return ni * nj * nk, (nj * nk, nk, 1), lambda ptr: 0
    if layout == "jfirst":
        return ni * nj * nk, (nj, 1, ni * nj), lambda ptr: 0
    raise ValueError(layout)


def host_view(host_flat: np.ndarray, shape, strides, offset: int) -> np.ndarray:
    isz = host_flat.itemsize
    return np.lib.stride_tricks.as_strided(host_flat[offset:], shape, tuple(s * isz for s in strides))


class Layout:
    """A device buffer of integers in one of the four layouts, kept as a FLAT tensor so that every byte of it can be compared."""

    def __init__(self, shape, layout: str, itemsize: int, align_i: int = 0):
        import torch

        tdt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[itemsize]
        numel, self.strides, offset = geometry(shape, layout, itemsize, align_i)
        self.flat = torch.empty(numel, dtype=tdt, device="cuda")
        self.offset = offset(self.flat.data_ptr())
        self.shape, self.itemsize = tuple(shape), itemsize
        self.view = torch.as_strided(self.flat, self.shape, self.strides, self.offset)

    def host_view(self, host_flat):
        return host_view(host_flat, self.shape, self.strides, self.offset)

    def upload(self, host_flat):
        import torch

        self.flat.copy_(torch.from_numpy(host_flat))

    def download(self):
        return self.flat.cpu().numpy()


def sentinel_image(numel: int, itemsize: int) -> np.ndarray:
    return np.full(numel, SENTINEL[itemsize], dtype=NP_UINT[itemsize]).view(NP_INT[itemsize])


def random_image(numel: int, itemsize: int, rng) -> np.ndarray:
    info = np.iinfo(NP_INT[itemsize])
    return rng.integers(info.min, info.max, size=numel, dtype=NP_INT[itemsize], endpoint=True)


class Dev:
    """An array on the device in one of the four layouts, as a FLAT buffer whose every byte is known: ``values`` in the view, a
    NaN-payload sentinel everywhere else (``values=None``: everywhere).  One ghost row / column behind the high I / J end of what
    the product is given (``given``): the array ends there for the product, the buffer does not."""

    def __init__(self, shape, dtype, layout, values=None, align_i=0):
        import torch

        self.dtype = np.dtype(dtype)
        isz = self.dtype.itemsize
        self.lay = Layout(shape, layout, isz, align_i)
        self.image = sentinel_image(self.lay.flat.numel(), isz)
        if values is not None:
            self.host(self.image)[...] = values
        self.lay.upload(self.image)
        self.given = self.lay.view.view({4: torch.float32, 8: torch.float64}[isz])[:-1, :-1]

    def host(self, image):
        """The view of a host image of the flat buffer, as floats."""
        return self.lay.host_view(image.view(self.dtype))

    def assert_unchanged(self, what):
        assert np.array_equal(self.lay.download(), self.image), f"{what} changed"

    def assert_box(self, box, want_box, what):
        """The box holds ``want_box`` (NaN as NaN), every other byte of the buffer what it held.  Returns the box as it is."""
        got = self.lay.download()
        want = self.image.copy()
        self.host(want)[box] = want_box
        inside = np.zeros(want.shape, dtype=bool)
        self.lay.host_view(inside)[box] = True
        both_nan = np.isnan(got.view(self.dtype)) & np.isnan(want.view(self.dtype))
        ok = (got == want) | (inside & both_nan)
        if not ok.all():
            bad = np.flatnonzero(~ok)
            raise AssertionError(f"{what}: {bad.size} items of the whole buffer differ ({int((~ok & inside).sum())} of them in the box), "
                                 f"first at flat index {bad[:6].tolist()} (view offset {self.lay.offset}, strides {self.lay.strides}); "
                                 f"got {got.view(self.dtype)[bad[:6]].tolist()}, want {want.view(self.dtype)[bad[:6]].tolist()}")
        return np.array(self.host(got)[box])


class Line:
    """A 1-d array on the device (a ``Field[K]`` of edges, a coefficient along a line), cast to ``dtype`` where one is given."""

    def __init__(self, values, dtype=None):
        import torch

        self.values = np.ascontiguousarray(values, dtype=dtype)
        self.given = torch.from_numpy(self.values).cuda()

    def assert_unchanged(self, what):
        assert np.array_equal(self.given.cpu().numpy().view(np.uint8), self.values.view(np.uint8)), f"{what} changed"
