"""The arithmetic contract of ``gt4mi_line_filter`` (include/gt4py_amd.h) restated twice: :func:`filter_line` / :func:`spectrum_line` in
plain Python, one butterfly at a time on numpy float64 scalars (numpy rounds every scalar operation once and fuses nothing), and
:func:`filter_along` / :func:`spectrum_along` in vectorised numpy, the lines side by side, which is what the tests use on whole boxes.
tests/test_line_filter.py compares the two with each other and with ``numpy.fft``.  Test infrastructure; imports no product code."""

from __future__ import annotations

import numpy as np


def twiddles(n: int):
    """``(wr, wi)`` for j < n/2: cos(2 pi j / n) and -sin(2 pi j / n) from numpy in float64, w[0] = (1, 0) and w[n/4] = (0, -1) exact."""
    j = np.arange(n // 2, dtype=np.float64)
    wr, wi = np.cos(2.0 * np.pi * j / n), -np.sin(2.0 * np.pi * j / n)
    wr[0], wi[0] = 1.0, 0.0
    if n >= 4:
        wr[n // 4], wi[n // 4] = 0.0, -1.0
    return wr, wi


def bitrev(n: int) -> np.ndarray:
    """bitrev_L(p) for p < n = 2 ** L."""
    L = n.bit_length() - 1
    p = np.arange(n)
    m = np.zeros(n, dtype=np.int64)
    for b in range(L):
        m |= ((p >> b) & 1) << (L - 1 - b)
    return m


def _check_length(n: int) -> None:
    assert 2 <= n <= 4096 and n & (n - 1) == 0, n


# ---- plain Python: one line, one butterfly at a time ---------------------------------------------------------------------------
def forward_line(x):
    """The forward transform of one line (a 1-d array of float32 or float64): two lists of numpy float64 scalars, bit-reversed order."""
    n = len(x)
    _check_length(n)
    wr, wi = twiddles(n)
    re, im = [np.float64(v) for v in x], [np.float64(0.0)] * n
    with np.errstate(all="ignore"):
        h = n // 2
        while h >= 1:
            for start in range(0, n, 2 * h):
                for j in range(h):
                    p, q = start + j, start + j + h
                    cr, ci = wr[j * n // (2 * h)], wi[j * n // (2 * h)]
                    ur, ui = re[p] - re[q], im[p] - im[q]
                    re[p], im[p] = re[p] + re[q], im[p] + im[q]
                    re[q], im[q] = cr * ur - ci * ui, cr * ui + ci * ur
            h //= 2
    return re, im


def spectrum_line(x):
    """``X[m]`` for m <= n/2 as (real parts, imaginary parts), two float64 arrays of n/2 + 1."""
    n = len(x)
    re, im = forward_line(x)
    m = bitrev(n)
    keep = m <= n // 2
    out_r, out_i = np.empty(n // 2 + 1), np.empty(n // 2 + 1)
    out_r[m[keep]], out_i[m[keep]] = np.array(re)[keep], np.array(im)[keep]
    return out_r, out_i


def filter_line(x, response):
    """One line filtered: an array of ``x``'s dtype.  ``response``: n/2 + 1 float64."""
    x = np.asarray(x)
    n = len(x)
    wr, wi = twiddles(n)
    re, im = forward_line(x)
    m = bitrev(n)
    with np.errstate(all="ignore"):
        for p in range(n):
            r = np.float64(response[min(m[p], n - m[p])])
            re[p], im[p] = re[p] * r, im[p] * r
        h = 1
        while h <= n // 2:
            for start in range(0, n, 2 * h):
                for j in range(h):
                    p, q = start + j, start + j + h
                    cr, ci = wr[j * n // (2 * h)], wi[j * n // (2 * h)]
                    tr, ti = cr * re[q] + ci * im[q], cr * im[q] - ci * re[q]
                    ar, ai = re[p], im[p]
                    re[p], im[p] = ar + tr, ai + ti
                    re[q], im[q] = ar - tr, ai - ti
            h *= 2
        scale = np.float64(1.0) / np.float64(n)
        return np.array([v * scale for v in re]).astype(x.dtype)


# ---- numpy: the lines side by side, along axis 0 ---------------------------------------------------------------------------------
def forward(x):
    """The forward transform along axis 0 of ``x`` (n, ...): (re, im) float64 arrays of that shape, bit-reversed order along axis 0."""
    x = np.asarray(x)
    n = x.shape[0]
    _check_length(n)
    wr, wi = twiddles(n)
    tail = (1,) * (x.ndim - 1)
    re, im = x.astype(np.float64), np.zeros(x.shape)
    with np.errstate(all="ignore"):
        h = n // 2
        while h >= 1:
            r, i = re.reshape((n // (2 * h), 2, h) + x.shape[1:]), im.reshape((n // (2 * h), 2, h) + x.shape[1:])
            cr, ci = wr[:: n // (2 * h)].reshape((1, h) + tail), wi[:: n // (2 * h)].reshape((1, h) + tail)
            ur, ui = r[:, 0] - r[:, 1], i[:, 0] - i[:, 1]
            ar, ai = r[:, 0] + r[:, 1], i[:, 0] + i[:, 1]
            r[:, 0], i[:, 0] = ar, ai
            r[:, 1], i[:, 1] = cr * ur - ci * ui, cr * ui + ci * ur
            h //= 2
    return re, im


def spectrum(x):
    """``(re, im)`` of wavenumbers 0 .. n/2 along axis 0 of ``x`` (n, ...): float64 arrays (n/2 + 1, ...)."""
    n = np.asarray(x).shape[0]
    re, im = forward(x)
    at = np.argsort(bitrev(n))[: n // 2 + 1]  # the slot that holds wavenumber m
    return re[at], im[at]


def filter(x, response):  # noqa: A001
    """``x`` (n, ...) filtered along axis 0; ``response`` (n/2 + 1, ...) float64 broadcasts against it.  Returns ``x``'s dtype."""
    x = np.asarray(x)
    n = x.shape[0]
    wr, wi = twiddles(n)
    tail = (1,) * (x.ndim - 1)
    re, im = forward(x)
    m = bitrev(n)
    response = np.asarray(response, dtype=np.float64)
    response = response.reshape(response.shape + (1,) * (x.ndim - response.ndim))
    with np.errstate(all="ignore"):
        r = response[np.minimum(m, n - m)]
        re, im = re * r, im * r
        h = 1
        while h <= n // 2:
            a, b = re.reshape((n // (2 * h), 2, h) + x.shape[1:]), im.reshape((n // (2 * h), 2, h) + x.shape[1:])
            cr, ci = wr[:: n // (2 * h)].reshape((1, h) + tail), wi[:: n // (2 * h)].reshape((1, h) + tail)
            tr, ti = cr * a[:, 1] + ci * b[:, 1], cr * b[:, 1] - ci * a[:, 1]
            ar, ai = a[:, 0].copy(), b[:, 0].copy()
            a[:, 0], b[:, 0] = ar + tr, ai + ti
            a[:, 1], b[:, 1] = ar - tr, ai - ti
            h *= 2
        return (re * (np.float64(1.0) / np.float64(n))).astype(x.dtype)


def _response_lines_first(response, axis):
    """A response ``(nh,)`` or ``(ea, eb, nh)`` (ea, eb along the two other axes in IJK order) with wavenumbers first."""
    response = np.asarray(response, dtype=np.float64)
    return response if response.ndim == 1 else np.moveaxis(response, 2, 0)


def filter_along(x, axis, response):
    """:func:`filter` along ``axis`` of the IJK array ``x``; the response is ``(nh,)`` or ``(ea, eb, nh)``, an extent of 1 broadcasts."""
    out = filter(np.moveaxis(np.asarray(x), axis, 0), _response_lines_first(response, axis))
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def spectrum_along(x, axis):
    """``(2, ea, eb, nh)`` float64: the rows of one field of a ``LineSpectrum`` result."""
    re, im = spectrum(np.moveaxis(np.asarray(x), axis, 0))
    return np.ascontiguousarray(np.stack([np.moveaxis(re, 0, 2), np.moveaxis(im, 0, 2)]))


def power(coefficients, n):
    """``|X[m]|^2 / n^2`` of complex coefficients (..., nh), with the factor 2 for 0 < m < n/2."""
    p = (coefficients.real * coefficients.real + coefficients.imag * coefficients.imag) / (float(n) * float(n))
    p[..., 1: n // 2] *= 2.0
    return p


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def same_bits(x, y):
    """Elementwise: the same bits, or NaN on both sides."""
    x, y = np.asarray(x), np.asarray(y)
    return (bits(x) == bits(y)) | (np.isnan(x) & np.isnan(y))
