"""Parity of the POA chain kernel with the oracle on chains built for the RARE paths of its incremental re-sort (tests/resort_cases.py).

topo_sort_incremental re-sorts the graph after almost every read by replaying the Kahn walk over a 64-row window from a cut of the old order; its order, cut
flags and `remain` must equal the full re-sort's and oracle/poa.c's, and whatever it cannot handle it must refuse before it writes.  Every other input of the
suite asks it for a walk of at most a dozen rows (tests/test_resort_cases_oracle.py holds the census, the converse, and checks on the CPU that every chain here
lands in the class its row names).  Every row of CASES runs through lcd.poa_batch under its environment and under each of its further ones -- the incremental
re-sort off (LCD_DBG=1024), the other layouts of the full re-sort that the refused reads then take (64, 384), the generic rows (8) -- and EVERY run is
compared with the oracle: status, n_cons, msa_len, every consensus, every cluster, every MSA row byte for byte.  The default and LCD_DBG=1024 are thereby both
held to the oracle, not merely to each other."""
import pytest

import resort_cases as R
from test_gpu_poa_ties import _same

pytestmark = pytest.mark.gpu

_SWITCHES = sorted({k for c in R.CASES for env in [c["env"]] + c["also"] for k in env})


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_poa_resort_chain_matches_oracle(lcd, oracle, case, monkeypatch):
    exp, census = R.case_oracle(case)
    if case["mode"] == 0:
        assert exp["n_cons"] == 1
    opt = lcd.default_opt()
    opt.is_ont = case["is_ont"]
    job = [dict(mode=case["mode"], reads=R.chain_reads(case))]
    for env in [case["env"]] + case["also"]:
        with monkeypatch.context() as m:
            for k in _SWITCHES:
                m.delenv(k, raising=False)
            for k, v in env.items():      # (the switches are read at every call)
                m.setenv(k, v)
            got = lcd.poa_batch(job, opt)[0]
        _same(got, exp, (case["name"], env, R.census_line(census)))
