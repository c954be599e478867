"""The key blobs at their consumers on the CPU interpreter (tests/hipemu); cases in tests/key_blob_cases.py.  Plus the reader of
owshen_amd/csrc/key_blob.h alone, compiled with the address and undefined-behaviour sanitizers into a program of its own."""
import hashlib
import os
import subprocess

import pytest

from tests import key_blob_cases as cases

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ectx():
    from tests import emu
    c = emu.Ctx()
    yield c
    c.close()


def test_emu_k1_meets_every_padding(ectx):
    cases.case_k1_meets_every_padding(ectx)


@pytest.mark.parametrize("consumer", cases.PK_CONSUMERS)
def test_emu_outcomes_of_malformed_proving_keys(ectx, consumer):
    cases.case_outcomes(ectx, "pk", consumer)


@pytest.mark.parametrize("consumer", cases.VK_CONSUMERS)
def test_emu_outcomes_of_malformed_verifying_keys(ectx, consumer):
    cases.case_outcomes(ectx, "vk", consumer)


def test_emu_blob_digests(ectx):
    cases.case_digests(ectx)


@pytest.mark.parametrize("consumer", sorted(cases.CALLS))
def test_emu_unaligned_blobs(ectx, consumer):
    cases.case_unaligned(ectx, consumer)


def test_emu_pk_info_is_the_header(ectx):
    cases.case_pk_info(ectx)


def test_reader_alone_under_sanitizers(tmp_path):
    """key_blob.h as a host program of its own (tests/key_blob_reader.cpp): K1 parsed and CSR-checked at byte offsets 0..7,
    -fsanitize=address,undefined -- a misaligned word load or a read past the blob ends the program"""
    k1 = os.path.join(cases.GOLDEN, "k1_pk.bin")
    with open(k1, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == cases.golden("digests.json")["og_setup K1 pk"]
    exe = str(tmp_path / "key_blob_reader")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-attributes",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(_ROOT, "tests", "hipemu"), "-I", os.path.join(_ROOT, "owshen_amd", "csrc"),
                           os.path.join(_ROOT, "tests", "key_blob_reader.cpp"), "-o", exe])
    run = subprocess.run([exe, k1], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.split() == ["ok", "8", "offsets"]
