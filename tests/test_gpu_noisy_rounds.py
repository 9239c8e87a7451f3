"""lcd_chunks_noisy_rounds on the MI355X: device chunks from "first round done" to the fixed point of collect_var_main's noisy-region loop
(src/collect_var.c:2946-2977), against the loop composed from the existing oracles (pass_plan_common.oracle_rounds) and against the same loop stepped through
the library's single exports (pass_plan_common.stepped_rounds)."""
import numpy as np
import pytest

import clean_vars_common as cc
import pass_plan_common as pc
from test_gpu_clean_vars import chunk_args, device_chunk

pytestmark = pytest.mark.gpu


def first_round(lcd, oracle, ch, is_ont=0):
    """records -> device chunk -> lcd_chunk_clean_vars -> K5 over the clean categories: the driver's inputs, and the oracle's side of the same state"""
    from longcalld_amd import jobs
    digs = cc.read_digars(ch, oracle, is_ont=is_ont)
    a = chunk_args(lcd, ch, digs)
    low = lcd.sdust(ch["ref"], 5, 20)                      # chunk->low_comp_cr in reference coordinates (src/bam_utils.c:1573-1581)
    a["low_comp"] = np.stack([ch["ref_beg"] + low[:, 0] - 1, ch["ref_beg"] + low[:, 1] - 1], 1).astype(np.int64)
    ci = cc.chunk_inputs(ch, digs)
    a["pre_regs"] = lcd.pre_process_noisy_regs(ci["chunk_noisy"], a["low_comp"], ci["read_beg"], ci["read_end"], ci["read_ivs"])
    dev = device_chunk(lcd, ch)
    opt = lcd.clean_opt(is_ont)
    cv = dev.clean_vars(**a, opt=opt)
    want = cc.run_oracle(ch, digs, opt, pre_regs=a["pre_regs"], low_comp=a["low_comp"], ordered=a["ordered_read_ids"])
    cc.same_clean_vars(cv, want)
    ordered = a["ordered_read_ids"]
    skipped = np.array([d["rc"] != 0 for d in digs], np.uint8)
    st = lcd.assign_hap_germline(lcd.clean_vars_hap_problem(cv, ordered, skipped, is_ont), jobs.GERMLINE_CLEAN)
    ex = oracle.assign_hap_germline(pc.py_hap_problem(want, ordered, skipped, is_ont), jobs.GERMLINE_CLEAN)
    pc.same_state(st, ex, pc.STATE_KEYS)
    return dict(ch=ch, digs=digs, dev=dev, cv=cv, want=want, st=st, ex=ex, ordered=ordered, skipped=skipped)


def _item(f, cv=None):
    return dict(cv=cv if cv is not None else f["cv"], state=f["st"], ordered_read_ids=f["ordered"], is_skipped=f["skipped"], ref=f["ch"]["ref"], ref_beg=f["ch"]["ref_beg"],
                is_ont=f["ch"].get("is_ont", 0))


def test_driver_on_the_real_hg002_chunk_equals_the_oracle_loop_and_the_stepped_loop(lcd, oracle):
    """The real HG002 chunk with max_noisy_reg_len = 3000 (the cut tests/test_gpu_chunk_noisy_pass.py uses, so that the oracle stays quick).  This chunk converges
    in one productive pass plus the empty one: 74 of its 75 regions are resolved in the first pass (the last one is longer than the cut and done without a
    variant), the table grows from 330 to 534 variants, and the second pass plans nothing and ends the loop.  The state a merge returns feeding a later
    productive pass is the subject of test_second_pass_resolves_a_region_left_over_from_the_first below."""
    f = first_round(lcd, oracle, cc.events_chunk())
    popt = lcd.pass_opt(max_noisy_reg_len=3000)
    before = lcd.copy_counters()
    got = lcd.chunks_noisy_rounds([f["dev"]], [_item(f)], popt=popt)[0]
    assert lcd.copy_counters() == before                                         # no digar and no base crossed PCIe
    want = pc.oracle_rounds(oracle, f["ch"], f["digs"], f["want"], f["ex"], f["ordered"], f["skipped"], max_len=3000)
    print("passes", want["n_passes"], "productive", want["productive"], "resolved per pass", want["resolved"], "done", int(want["done"].sum()), "of", len(want["done"]),
          "vars", f["want"]["n_vars"], "->", want["cv"]["n_vars"])
    pc.same_rounds(got, want)
    step = pc.stepped_rounds(lcd, f["dev"], f["cv"], f["st"], f["ordered"], f["skipped"], f["ch"]["ref"], f["ch"]["ref_beg"], popt)
    pc.same_rounds(got, step)
    pc.same_state(got["state"], step["state"])
    assert got["n_passes"] == 2 and want["productive"] == 1 and got["cv"]["n_vars"] > f["cv"]["n_vars"] and got["done"].all()
    assert (got["first_to_final"] >= 0).all() and (np.diff(got["first_to_final"]) > 0).all()
    assert len(got["state"]["var_phase_set"]) == got["cv"]["n_vars"]
    f["dev"].close()


def test_second_pass_resolves_a_region_left_over_from_the_first(lcd, oracle):
    """pass_plan_common.two_pass_chunk: the second region needs both haplotypes phased, which only the first pass's variants provide"""
    f = first_round(lcd, oracle, pc.two_pass_chunk())
    assert len(f["cv"]["regs"]) == 2 and (f["st"]["haps"] == 0).all()             # nothing is phased after the clean-category K5 call
    got = lcd.chunks_noisy_rounds([f["dev"]], [_item(f)])[0]
    want = pc.oracle_rounds(oracle, f["ch"], f["digs"], f["want"], f["ex"], f["ordered"], f["skipped"])
    assert want["resolved"] == [1, 1, 0] and want["productive"] == 2
    pc.same_rounds(got, want)
    step = pc.stepped_rounds(lcd, f["dev"], f["cv"], f["st"], f["ordered"], f["skipped"], f["ch"]["ref"], f["ch"]["ref_beg"], lcd.pass_opt())
    pc.same_rounds(got, step)
    pc.same_state(got["state"], step["state"])
    assert got["n_passes"] == 3 and got["done"].tolist() == [1, 1] and got["cv"]["n_vars"] == 17 and sorted(set(got["state"]["haps"].tolist())) == [1, 2]
    f["dev"].close()


def test_one_read_region_stays_open_after_one_pass_and_changes_nothing(lcd, oracle):
    ch = cc.make_diploid_chunk(11, ref_len=6000, depth=6)
    f = first_round(lcd, oracle, ch)
    info = f["dev"].read_info()
    # a region at the far left end that only the first read overlaps (the second read begins behind it)
    last = int(np.argmin(info["beg"]))
    second = int(np.sort(info["beg"])[1])
    assert info["status"][last] == 0 and second - info["beg"][last] >= 100
    cv = dict(f["cv"]); cv["regs"] = np.array([[int(info["beg"][last]) + 10, second - 1, 1]], np.int64)
    plan = lcd.plan_pass(f["dev"], cv["regs"], [0], f["ordered"], f["skipped"], ch["ref_beg"], ch["ref_beg"] + len(ch["ref"]) - 1)
    assert plan["status"].tolist() == [pc.SUBMIT] and plan["read_ids"].tolist() == [last]
    got = lcd.chunks_noisy_rounds([f["dev"]], [_item(f, cv)])[0]
    assert got["done"].tolist() == [0] and got["n_passes"] == 1
    cc.same_clean_vars(got["cv"], cv)
    pc.same_state(got["state"], f["st"])
    assert (got["first_to_final"] == np.arange(cv["n_vars"])).all()
    f["dev"].close()


def test_four_chunks_in_one_driver_call_equal_four_single_calls(lcd, oracle):
    fs = [first_round(lcd, oracle, cc.make_diploid_chunk(200 + i, ref_len=12000)) for i in range(4)]
    popt = lcd.pass_opt(max_noisy_reg_len=600)
    batch = lcd.chunks_noisy_rounds([f["dev"] for f in fs], [_item(f) for f in fs], popt=popt)
    assert any(b["cv"]["n_vars"] > f["cv"]["n_vars"] for b, f in zip(batch, fs))
    for f, b in zip(fs, batch):
        s = lcd.chunks_noisy_rounds([f["dev"]], [_item(f)], popt=popt)[0]
        pc.same_rounds(b, s)
        pc.same_state(b["state"], s["state"])
        f["dev"].close()
