"""CPU: argument handling of the batch decider's C-ABI entries.  Every check
runs before the context is looked at, so each error is reached here with a null
context and no device."""
import ctypes

import halo2_amd as H
import numpy as np
import pairing_ref as PR
import pairing_util as U
import pytest

ARG, UNSUPPORTED = -1, -4
BN254 = 2
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
SEED = bytes(range(32))


@pytest.fixture(scope="module")
def host_pairing():
    return H.Pairing(None, U.g2_words(PR.G2), U.g2_words(U.s_g2()))


def _outs():
    ok = np.full(2, 7, dtype=np.uint32)
    pair = np.full((2, 8), 9, dtype=np.uint64)
    used = ctypes.create_string_buffer(32)
    return ok, pair, used


def test_device_entry_checks_arguments_before_the_context(host_pairing):
    f = H.lib().pm_accum_decide_batch_device
    buf = np.zeros(64, dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    ok, pair, used = _outs()
    okp = ok.ctypes.data_as(_u32p)
    # B == 0 succeeds: ok = 1, the sums are the identity, the seed is reported
    assert f(None, None, 0, None, None, SEED, 0, okp, None, None, pair.ctypes.data_as(_u64p), used) == 0
    assert list(ok) == [1, 7] and not pair.any() and used.raw == SEED
    assert f(None, None, 0, None, None, None, 0, None, None, None, None, None) == 0
    ok[0] = 7
    assert f(None, None, 1, p, None, SEED, 0, okp, None, None, None, None) == ARG  # null pm_pairing
    assert f(None, host_pairing.h, 1, None, None, SEED, 0, okp, None, None, None, None) == ARG  # null input
    assert f(None, host_pairing.h, 1, p, None, SEED, 0, None, None, None, None, None) == ARG  # null out_ok
    assert f(None, host_pairing.h, (1 << 24) + 1, p, None, SEED, 0, okp, None, None, None, None) == UNSUPPORTED
    assert f(None, host_pairing.h, 1, p, None, SEED, 2, okp, None, None, None, None) == ARG  # unknown flag bit
    assert b"flag" in H.lib().pm_last_error()
    assert f(None, host_pairing.h, 1, p, None, SEED, 0x80000001, okp, None, None, None, None) == ARG
    assert f(None, host_pairing.h, 1, p, None, SEED, 1, okp, None, None, None, None) == ARG  # null context, last
    assert b"context" in H.lib().pm_last_error()
    assert not buf.any() and list(ok) == [7, 7]


def test_host_pointer_entry(host_pairing):
    f = H.lib().pm_accum_decide_batch
    q = np.zeros((1, 4, 8), dtype=np.uint64)
    qp = q.ctypes.data_as(_u64p)
    ok, pair, used = _outs()
    okp = ok.ctypes.data_as(_u32p)
    assert f(None, None, 0, None, None, None, 0, okp, None, None, None, None) == 0 and list(ok) == [1, 7]
    ok[0] = 7
    assert f(None, None, 1, qp, None, SEED, 0, okp, None, None, None, None) == ARG
    assert f(None, host_pairing.h, 1, None, None, SEED, 0, okp, None, None, None, None) == ARG
    assert f(None, host_pairing.h, 1, qp, None, SEED, 0, None, None, None, None, None) == ARG
    assert f(None, host_pairing.h, (1 << 24) + 1, qp, None, SEED, 0, okp, None, None, None, None) == UNSUPPORTED
    assert f(None, host_pairing.h, 1, qp, None, SEED, 4, okp, None, None, None, None) == ARG
    assert f(None, host_pairing.h, 1, qp, None, SEED, 0, okp, None, None, None, None) == ARG
    assert b"context" in H.lib().pm_last_error()
    assert list(ok) == [7, 7]


def test_host_entry(host_pairing):
    f = H.lib().pm_accum_decide_batch_host
    q = np.zeros((1, 4, 8), dtype=np.uint64)
    qp = q.ctypes.data_as(_u64p)
    ok, pair, used = _outs()
    okp = ok.ctypes.data_as(_u32p)
    assert f(None, 0, None, None, None, 0, okp, None, None, None, None) == 0 and list(ok) == [1, 7]
    ok[0] = 7
    assert f(None, 1, qp, None, SEED, 0, okp, None, None, None, None) == ARG
    assert f(host_pairing.h, 1, None, None, SEED, 0, okp, None, None, None, None) == ARG
    assert f(host_pairing.h, 1, qp, None, SEED, 0, None, None, None, None, None) == ARG
    assert f(host_pairing.h, (1 << 24) + 1, qp, None, SEED, 0, okp, None, None, None, None) == UNSUPPORTED
    assert f(host_pairing.h, 1, qp, None, SEED, 2, okp, None, None, None, None) == ARG
    assert list(ok) == [7, 7]
    # the all-identity quad is accepted; every optional output may be null; without the flag
    # out_item_ok is not touched
    item = np.full(1, 5, dtype=np.uint32)
    assert f(host_pairing.h, 1, qp, None, SEED, 0, okp, item.ctypes.data_as(_u32p), None, None, None) == 0
    assert list(ok) == [1, 7] and item[0] == 5
    assert f(host_pairing.h, 1, qp, None, None, 1, okp, item.ctypes.data_as(_u32p), None,
             pair.ctypes.data_as(_u64p), used) == 0
    assert item[0] == 1 and not pair.any() and used.raw != bytes(32)


def test_verify_proofs_batch_entry(host_pairing):
    f = H.lib().pm_verify_proofs_batch_device
    buf = np.zeros(64, dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    vk = buf.ctypes.data_as(_u64p)
    ok, pair, used = _outs()
    okp = ok.ctypes.data_as(_u32p)
    pr = host_pairing.h

    def call(curve=BN254, B=1, quads=p, status=p, pairing=pr, flags=0, out_ok=okp):
        return f(None, curve, None, B, vk, p, 0, None, p, quads, None, status, pairing, SEED, flags, out_ok, None,
                 None, None)

    assert call(curve=0) == ARG and b"BN254" in H.lib().pm_last_error()  # Pallas
    assert call(B=0) == 0 and list(ok) == [1, 7]
    ok[0] = 7
    assert call(pairing=None) == ARG
    assert call(quads=None) == ARG
    assert call(out_ok=None) == ARG
    assert call(B=(1 << 24) + 1) == UNSUPPORTED
    assert call(flags=8) == ARG
    assert call(status=None) == ARG and b"d_out_status" in H.lib().pm_last_error()
    assert call() == ARG and b"context" in H.lib().pm_last_error()  # null context, looked at last
    assert not buf.any() and list(ok) == [7, 7]
