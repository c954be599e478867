"""Redeem-statement cases shared by the CPU-interpreter run and the GPU run: the cases of tests/send_cases.py, which are written once
over a description of the statement, bound to the redeem statement (tests/redeem_spec.py).  The cases that need both statements --
the one spent set, the two hops through the pool -- live in tests/send_cases.py."""
import functools
import types

from tests import redeem_spec
from tests import send_cases as base

REDEEM = types.SimpleNamespace(
    name="redeem", spec=redeem_spec, n_pub=7, part="amount_out", part_wire=4, change_wire=11, leaf_wire=7, leaf_commitment="change_commitment",
    fields=("x", "amount", "recipient", "amount_out", "token", "chain_id", "change_commitment", "index"),
    extra=("recipient",), wrong_key="split", leaf_forge="change_leaf", token_forge="change_asset_token")

edge_inputs = functools.partial(base.edge_inputs, REDEEM)
case_redeem_r1cs_and_witness_match_spec = functools.partial(base.case_r1cs_and_witness_match_spec, REDEEM)
case_redeem_end_to_end = functools.partial(base.case_end_to_end, REDEEM)
case_redeem_batch_130_verifies = functools.partial(base.case_batch_130_verifies, REDEEM)
case_redeem_forgeries_are_unprovable = functools.partial(base.case_forgeries_are_unprovable, REDEEM)
case_redeem_the_theft_is_closed = functools.partial(base.case_the_theft_is_closed, REDEEM)
case_redeem_record_boundary = functools.partial(base.case_record_boundary, REDEEM)
case_redeem_second_slab = functools.partial(base.case_second_slab, REDEEM)
key = functools.partial(base._key, REDEEM)
