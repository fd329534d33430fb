"""scripts/isa_compare.py on synthetic assembly text (no compiler, no GPU): the comparison that
guards a change meant to leave the shipped kernels as they are must pass streams that differ only
in label numbers and the blanks that pad them, and must report a changed instruction, a removed
kernel and a changed register count."""
import importlib.util
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_compare", os.path.join(REPO, "scripts", "isa_compare.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)


_nfunc = [0]


def kernel(name, body, vgpr=32, sgpr=16, lds=0, scratch=0, figures=None):
    if figures is None:
        figures = (f"\t\t.amdhsa_group_segment_fixed_size {lds}\n\t\t.amdhsa_private_segment_fixed_size {scratch}\n"
                   f"\t\t.amdhsa_next_free_vgpr {vgpr}\n\t\t.amdhsa_next_free_sgpr {sgpr}\n")
    _nfunc[0] += 1   # the compiler numbers the end labels through the file
    end = f".Lfunc_end{_nfunc[0]}"
    return (f"\t.globl\t{name}\n{name}:                 ; @{name}\n; %bb.0:\n{body}\ts_endpgm\n"
            f"\t.section\t.rodata,\"a\",@progbits\n\t.amdhsa_kernel {name}\n{figures}"
            f"\t\t.amdhsa_float_round_mode_32 0\n\t.end_amdhsa_kernel\n\t.text\n"
            f"{end}:\n\t.size\t{name}, {end}-{name}\n")


def body(label, pad="", add="v_add_f64 v[0:1], v[0:1], v[2:3]"):
    return (f"\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n\ts_waitcnt lgkmcnt(0)\n"
            f".LBB0_{label}:{pad}                     ; =>This Inner Loop Header: Depth=1\n"
            f"\t{add}\n\ts_cbranch_scc1 .LBB0_{label}{pad}\n; %bb.2:\n\tglobal_store_dwordx2 v4, v[0:1], s[0:1]\n")


A = "_Z1aILi0EEv4Args"
B = "_Z1bILi1EEv4Args"


def test_label_numbers_and_padding_are_not_a_difference():
    # one file cut into two: the labels are renumbered (7 -> 112) and padded differently
    before = [kernel(A, body(7)) + kernel(B, body(8))]
    after = [kernel(B, body(112, pad="  ")), kernel(A, body(3, pad=" \t"))]
    res = isa.compare(before, after)
    assert res["ok"], res
    assert (res["before"], res["after"]) == (2, 2)
    assert not (res["changed"] or res["swapped"] or res["resources"] or res["removed"] or res["new"])


def test_changed_instruction_is_reported():
    before = [kernel(A, body(1)) + kernel(B, body(2))]
    after = [kernel(A, body(1)), kernel(B, body(2, add="v_add_f64 v[0:1], v[0:1], v[4:5]"))]
    res = isa.compare(before, after)
    assert not res["ok"]
    assert res["changed"] == [B] and not res["swapped"] and not res["resources"]
    # an extra wait is a change too, whatever else is equal
    after = [kernel(A, body(1, add="s_waitcnt vmcnt(0)\n\tv_add_f64 v[0:1], v[0:1], v[2:3]")), kernel(B, body(2))]
    res = isa.compare(before, after)
    assert not res["ok"] and res["changed"] == [A]


def test_change_after_an_early_exit_is_reported():
    # a kernel with an early exit holds two s_endpgm: the stream runs to the end label, not to the first
    early = "\ts_cbranch_execz .LBB0_9\n\ts_endpgm\n.LBB0_9:\n"
    before = [kernel(A, early + body(1))]
    assert isa.compare(before, [kernel(A, early + body(4))])["ok"]
    assert len(isa.kernels(before[0])[A]) > len(isa.kernels(kernel(A, body(1)))[A])
    res = isa.compare(before, [kernel(A, early + body(1, add="v_add_f64 v[0:1], v[0:1], v[4:5]"))])
    assert not res["ok"] and res["changed"] == [A]


def test_missing_resource_figure_is_reported():
    # no figure on either side is not "equal": nothing was compared
    bare = "\t\t.amdhsa_next_free_vgpr 32\n\t\t.amdhsa_next_free_sgpr 16\n\t\t.amdhsa_group_segment_fixed_size 0\n"
    res = isa.compare([kernel(A, body(1), figures=bare)], [kernel(A, body(1), figures=bare)])
    assert not res["ok"] and not res["resources"]
    assert res["missing"] == [("before", A, "private_segment_fixed_size"), ("after", A, "private_segment_fixed_size")]


def test_commutative_operand_swap_is_listed_apart():
    before = [kernel(A, body(1))]
    after = [kernel(A, body(1, add="v_add_f64 v[0:1], v[2:3], v[0:1]"))]
    res = isa.compare(before, after)
    assert res["ok"] and not res["changed"]
    (name, swaps), = res["swapped"]
    assert name == A and len(swaps) == 1
    assert swaps[0][1:] == ("v_add_f64 v[0:1], v[0:1], v[2:3]", "v_add_f64 v[0:1], v[2:3], v[0:1]")
    # a subtraction's operands exchanged is another result: a change
    before = [kernel(A, body(1, add="v_sub_f64 v[0:1], v[0:1], v[2:3]"))]
    after = [kernel(A, body(1, add="v_sub_f64 v[0:1], v[2:3], v[0:1]"))]
    res = isa.compare(before, after)
    assert not res["ok"] and res["changed"] == [A]


def test_removed_and_new_kernels_are_reported():
    before = [kernel(A, body(1)) + kernel(B, body(2))]
    res = isa.compare(before, [kernel(A, body(1))])
    assert not res["ok"] and res["removed"] == [B] and not res["new"] and not res["changed"]
    res = isa.compare([kernel(A, body(1))], before)
    assert not res["ok"] and res["new"] == [B] and not res["removed"]
    # the same kernel in two files of one side is an error of the split, not a match
    res = isa.compare(before, [kernel(A, body(1)), kernel(A, body(1)) + kernel(B, body(2))])
    assert not res["ok"] and res["twice"] == [A]


def test_changed_register_count_is_reported():
    before = [kernel(A, body(1), vgpr=128) + kernel(B, body(2), lds=4096)]
    after = [kernel(A, body(1), vgpr=132), kernel(B, body(2), lds=4096)]
    res = isa.compare(before, after)
    assert not res["ok"] and not res["changed"]
    (name, b, a), = res["resources"]
    assert name == A and b["next_free_vgpr"] == "128" and a["next_free_vgpr"] == "132"
    for field, kw in (("next_free_sgpr", "sgpr"), ("group_segment_fixed_size", "lds"),
                      ("private_segment_fixed_size", "scratch")):
        res = isa.compare([kernel(A, body(1))], [kernel(A, body(1), **{kw: 24})])
        assert not res["ok"] and res["resources"][0][2][field] == "24", field


def test_command_line_takes_several_files_a_side(tmp_path, capsys):
    files = {"b.s": kernel(A, body(1)) + kernel(B, body(2)), "a1.s": kernel(A, body(5)), "a2.s": kernel(B, body(6)),
             "a3.s": kernel(B, body(6), vgpr=40)}
    for n, t in files.items():
        (tmp_path / n).write_text(t)
    p = lambda n: str(tmp_path / n)
    assert isa.main([p("b.s"), p("a1.s"), p("a2.s")]) == 0
    assert isa.main([p("a1.s"), p("a2.s"), "--", p("b.s")]) == 0
    assert "kernels: 2 before, 2 after; changed 0" in capsys.readouterr().out
    assert isa.main([p("b.s"), p("a1.s"), p("a3.s")]) == 1
    assert "resources: " + B in capsys.readouterr().out
