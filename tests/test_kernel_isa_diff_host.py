"""tools/kernel_isa_diff.py --rename on synthetic assembly: a renamed kernel is compared like any other, with its own
name masked.  Host only: the parser reads two small texts; no compiler, no GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_isa_diff  # noqa: E402

ADD = "v_add_f64 v[0:1], v[0:1], v[2:3]"


def asm(names, op=ADD):
    """An assembly text in the compiler's layout: one kernel per name, the same code under each."""
    text, meta = ["\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\""], []
    for f, k in enumerate(names):
        text += [
            f"\t.section\t.text.{k},\"axG\",@progbits,{k},comdat",
            f"\t.globl\t{k} ; -- Begin function {k}",
            "\t.p2align\t8",
            f"\t.type\t{k},@function",
            f"{k}: ; @{k}",
            "; %bb.0:",
            "\ts_load_dwordx2 s[0:1], s[4:5], 0x0",
            f"\ts_cbranch_scc1 .LBB{f}_2",
            f"\t{op}",
            f".LBB{f}_2: ; in Loop: Header=BB{f}_1",
            "\ts_endpgm",
            "\t.section\t.rodata,\"a\",@progbits",
            f"\t.amdhsa_kernel {k}",
            "\t\t.amdhsa_next_free_vgpr 4",
            "\t.end_amdhsa_kernel",
            f"\t.section\t.text.{k},\"axG\",@progbits,{k},comdat",
            f".Lfunc_end{f}:",
            f"\t.size\t{k}, .Lfunc_end{f}-{k}",
            f"\t.set {k}.num_vgpr, 4",
        ]
        meta += ["  - .args:", "      - .offset:         0", "        .size:           8",
                 f"    .name:           {k}", f"    .symbol:         {k}.kd", "    .vgpr_count:     4"]
    return "\n".join(text + ["\t.amdgpu_metadata", "---", "amdhsa.kernels:"] + meta +
                     ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "...", "\t.end_amdgpu_metadata", ""])


@pytest.fixture
def run(tmp_path, capsys):
    def go(old, new, *args):
        (tmp_path / "old.s").write_text(old)
        (tmp_path / "new.s").write_text(new)
        status = kernel_isa_diff.main([str(tmp_path / "old.s"), str(tmp_path / "new.s"), "--source", "t.hip", *args])
        return status, capsys.readouterr().out
    return go


OLD = asm(["_Z3k_aPd", "_Z6k_a_fbPdi"])
NEW = asm(["_Z3k_aILb0EJEEvPd", "_Z3k_aILb1EJiEEvPdi"])
RENAMES = ("--rename", "_Z3k_aPd=k_aILb0E", "--rename", "k_a_fb=k_aILb1E")


def test_renamed_kernels_are_identical(run):
    status, out = run(OLD, NEW, *RENAMES)
    assert status == 0
    assert out.strip() == "t.hip: 2/2 identical"


def test_renamed_kernel_with_one_instruction_changed(run):
    changed = asm(["_Z3k_aILb0EJEEvPd", "_Z3k_aILb1EJiEEvPdi"], op="v_mul_f64 v[0:1], v[0:1], v[2:3]")
    status, out = run(OLD, changed, *RENAMES)
    assert status == 1
    assert "differs (body): _Z3k_aPd" in out and "differs (body): _Z6k_a_fbPdi" in out
    assert out.strip().endswith("t.hip: 0/2 identical  -- DIFFERENT")


def test_without_the_option_a_renamed_kernel_is_missing(run):
    status, out = run(OLD, NEW)
    assert status == 1
    assert "missing in NEW: _Z6k_a_fbPdi" in out and "only in NEW:    _Z3k_aILb1EJiEEvPdi" in out


@pytest.mark.parametrize("pair", ["k_b=k_aILb1E", "k_a_fb=k_b", "k_a=k_aILb1E", "k_a_fb"])
def test_unmatched_rename_is_an_error(run, pair, capsys):
    with pytest.raises(SystemExit) as e:      # no kernel, no kernel, two kernels (k_a is part of both), no '='
        run(OLD, NEW, "--rename", pair)
    assert e.value.code == 2
    assert "--rename" in capsys.readouterr().err
