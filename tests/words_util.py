"""TEST INFRASTRUCTURE: words of floats from the device against words from a restatement that ran on the host.  The two
agree on every word but one: a not-a-number that an operation made, not handed on."""
import numpy as np

HOST_NAN = {64: 0xFFF8000000000000, 32: 0xFFC00000}      # the NaN an x86 operation makes (0 / 0, inf - inf): quiet, the sign set
DEVICE_NAN = {64: 0x7FF8000000000000, 32: 0x7FC00000}    # ... and the one the device holds in its place: quiet, the sign clear


def device_words(want, bits=64):
    """the restatement's words with every HOST_NAN turned into DEVICE_NAN; nothing else moves"""
    want = np.asarray(want)
    assert want.dtype == (np.uint64 if bits == 64 else np.uint32), want.dtype
    return np.where(want == want.dtype.type(HOST_NAN[bits]), want.dtype.type(DEVICE_NAN[bits]), want)


def same_words(got, want, bits=64):
    """Words of floats against the restatement's, word for word - with one translation: where the restatement, run on the host,
    holds exactly the NaN its processor makes, the GPU must hold exactly the NaN its own makes (a fit's objective is no number
    on some of these tiny traces, on both sides; IEEE 754-2008, 6.3 leaves the sign of a made NaN to the processor).  Any other
    NaN - the all-ones word of a poisoned body among them - is a difference."""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.dtype == want.dtype == (np.uint64 if bits == 64 else np.uint32), (got.dtype, want.dtype)
    return got.shape == want.shape and np.array_equal(got, device_words(want, bits))


def expected_words(want, got, bits=64):
    """The words the device must hold, given the ones it does hold: the restatement's own, and - only where the restatement holds
    exactly HOST_NAN and the device exactly DEVICE_NAN - that one.  same_words() wants the translation at every HOST_NAN; that
    holds for the objectives it was written for and not in general: where a single operation makes the NaN (inf - inf in an
    emission term) gfx950 was seen to make the word x86 makes, sign set.  The two part where NaNs of different words meet in
    one addition - the processor's own in m_b next to the constant NaN hml_log returns for c_b - and the operand that wins is
    the compiler's choice on either side.  Any other pair of words is left as a difference for the comparison to find."""
    want, got = np.asarray(want), np.asarray(got)
    assert want.dtype == got.dtype == (np.uint64 if bits == 64 else np.uint32), (want.dtype, got.dtype)
    if want.size != got.size:
        return want
    t = want.dtype.type
    return np.where((want == t(HOST_NAN[bits])) & (got.reshape(want.shape) == t(DEVICE_NAN[bits])), t(DEVICE_NAN[bits]), want)


def same_or_translated(got, want, bits=64):
    """word for word: equal, or the one translation of expected_words()"""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    return got.shape == want.shape and np.array_equal(got, expected_words(want, got, bits))
