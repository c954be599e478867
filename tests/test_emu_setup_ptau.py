"""Key generation from a powers-of-tau file and the delta step on the CPU interpreter (tests/hipemu); cases in tests/ptau_cases.py."""
import random
import struct

import pytest

from tests import ptau_cases as cases


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("n_constraints,n_pub,extra_power", [(1, 0, 0), (25, 3, 0), (25, 3, 2)])
def test_emu_setup_ptau_equals_setup(ectx, n_constraints, n_pub, extra_power):
    cases.case_equals_setup_small(ectx, n_constraints, n_pub, extra_power)


def test_emu_setup_ptau_equals_setup_on_the_deposit_circuit(ectx):
    cases.case_equals_setup_deposit(ectx)


def test_emu_setup_ptau_long_and_empty_columns(ectx):
    cases.case_long_and_empty_columns(ectx)


def test_emu_pk_contribute(ectx):
    cases.case_contribute_small(ectx)


def test_emu_pk_contribute_to_an_imported_key(ectx):
    cases.case_contribute_imported(ectx)


def test_emu_ptau_key_proves_and_verifies(ectx):
    cases.case_key_works(ectx, n=3)


def test_emu_ptau_file_round_trip_and_cli(ectx, tmp_path):
    cases.case_file_round_trip(ectx, tmp_path)


def test_emu_setup_ptau_refusals(ectx):
    cases.case_refusals(ectx)
    cases.case_null_handles(ectx._lib)


def test_ptau_info_is_host_only(ectx):
    """og_ptau_info in the shipped library, on a host without a device: no context is ever made"""
    from owshen_amd import _lib
    cases.case_info(ectx, _lib.lib)
    cases.case_info(ectx, ectx._lib)
    cases.case_null_handles(_lib.lib)


def _mutants(good, rnd, n):
    secs, off = [], 12
    for _ in range(struct.unpack_from("<I", good, 8)[0]):
        sid, size = struct.unpack_from("<IQ", good, off)
        secs.append((sid, off, size))
        off += 12 + size
    for k in range(n):
        b = bytearray(good)
        kind = k % 6
        if kind == 0:                                   # a few random bit flips anywhere
            for _ in range(rnd.randrange(1, 4)):
                b[rnd.randrange(len(b))] ^= 1 << rnd.randrange(8)
        elif kind == 1:                                 # a run of random bytes
            o = rnd.randrange(len(b))
            for i in range(o, min(len(b), o + rnd.randrange(1, 80))):
                b[i] = rnd.randrange(256)
        elif kind == 2:                                 # truncation
            b = b[:rnd.randrange(len(b))]
        elif kind == 3:                                 # a section's length field rewritten
            _sid, o, size = rnd.choice(secs)
            struct.pack_into("<Q", b, o + 4, rnd.choice([0, 1, max(size, 1) - 1, size + 1, size * 2, 1 << 40, (1 << 64) - 1]))
        elif kind == 4:                                 # the header's n8 / power / ceremony power, or the section count
            hdr = next(o for sid, o, _ in secs if sid == 1) + 12
            o = rnd.choice([hdr, hdr + 36, hdr + 40, 8, 4])
            struct.pack_into("<I", b, o, rnd.choice([0, 1, 2, 3, 4, 5, 27, 28, 29, 64, 1 << 20, (1 << 31) - 1, (1 << 32) - 1]))
        else:                                           # a section id rewritten: a missing / duplicated / unknown section
            _sid, o, _size = rnd.choice(secs)
            struct.pack_into("<I", b, o, rnd.randrange(0, 16))
        yield kind, bytes(b)


def test_mutated_ptau_files_are_refused_or_make_a_loadable_key(ectx):
    """200 mutants of a valid file (power one above the domain, so that some bytes are never read): each is refused with
    OG_ERR_INVALID and a reason, or yields a key og_pk_load takes -- nothing else"""
    from owshen_amd import groth16 as g16, ptau
    from owshen_amd.api import OwshenGpuError
    r1cs = cases._small(5, 1)
    rnd = random.Random(20261018)
    good = cases.make_ptau(ectx, r1cs.log_d + 1, *cases._toxic(5))
    refused = made = 0
    for kind, data in _mutants(good, rnd, 200):
        try:
            pk, vk = ptau.setup(ectx, r1cs, data)
        except OwshenGpuError as e:
            assert e.code == -1 and "og_setup_ptau" in str(e), (kind, str(e))
            refused += 1
            continue
        made += 1
        g16.ProvingKey(ectx, pk).close()
        assert vk[:8] == b"OWVK0001"
    assert refused > 100 and made > 0 and refused + made == 200, (refused, made)
