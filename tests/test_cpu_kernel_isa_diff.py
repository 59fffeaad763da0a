"""not gpu: scripts/kernel_isa_diff.py, the comparison a refactor uses to show that no kernel changed, on three hand-written pairs of
assembly texts: equal up to comments and label numbers, one changed operand, one kernel renamed and one removed.  No hipcc needed;
the names are demangled where c++filt exists and stay mangled where it does not."""
import importlib.util
import io
import os
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_isa_diff", os.path.join(ROOT, "scripts", "kernel_isa_diff.py"))
kid = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kid)

FILT = shutil.which("c++filt") is not None
# (mangled, demangled): f<1, false, 0>() and f<1, false, true, 0>() -- the same kernel before and after a parameter is dropped -- and g()
F_NEW = ("_Z1fILi1ELb0ELi0EEvv", "void f<1, false, 0>()")
F_OLD = ("_Z1fILi1ELb0ELb1ELi0EEvv", "void f<1, false, true, 0>()")
G = ("_Z1gv", "g()")


def shown(k):
    return k[1] if FILT else k[0]


def kernel(k, fn, operand="v1", first_label=5, comment="x"):
    n = k[0]
    return """\t.text
\t.protected\t%(n)s ; -- Begin function %(n)s
\t.globl\t%(n)s
\t.p2align\t8
\t.type\t%(n)s,@function
%(n)s: ; @%(n)s
; %%bb.0:
\ts_load_dwordx2 s[4:5], s[0:1], 0x8   ; %(c)s
\tv_add_u32_e32 v0, v0, %(op)s
\ts_cbranch_execz .LBB%(fn)d_%(l0)d

.LBB%(fn)d_%(l1)d: ; =>This Inner Loop Header: Depth=1
\ts_cbranch_scc0 .LBB%(fn)d_%(l1)d
.LBB%(fn)d_%(l0)d:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel %(n)s
\t\t.amdhsa_next_free_vgpr 2
\t.end_amdhsa_kernel
\t.text
.Lfunc_end%(fn)d:
\t.size\t%(n)s, .Lfunc_end%(fn)d-%(n)s
                                        ; -- End function
\t.set %(n)s.num_vgpr, 2
; NumVgprs: 2
""" % {"n": n, "fn": fn, "op": operand, "l0": first_label, "l1": first_label - 2, "c": comment}


def run(old, new, **kw):
    out = io.StringIO()
    return kid.report(old, new, out=out, **kw), out.getvalue()


def test_comments_and_label_numbers_do_not_count():
    old = kernel(G, 0) + kernel(F_NEW, 1)
    new = kernel(F_NEW, 0, first_label=9, comment="another remark") + kernel(G, 7, first_label=4)      # other order, other numbers
    assert kid.compare(old, new) == ([], [], [], 2)
    status, text = run(old, new)
    assert status == 0 and text.splitlines() == ["compared 2  changed 0  removed 0  added 0"]


def test_a_changed_operand_is_reported():
    old = kernel(G, 0) + kernel(F_NEW, 1)
    new = kernel(G, 0) + kernel(F_NEW, 1, operand="v2")
    removed, added, changed, compared = kid.compare(old, new)
    assert (removed, added, compared) == ([], [], 2)
    assert changed == [(shown(F_NEW), len(kid.kernels(old)[F_NEW[0]]), len(kid.kernels(new)[F_NEW[0]]))]
    status, text = run(old, new)
    assert status == 1 and "changed: " + shown(F_NEW) in text
    # the label that moved is not what is reported: two different label orders are different streams too
    swapped = kernel(F_NEW, 1).replace("s_cbranch_scc0 .LBB1_3", "s_cbranch_scc0 .LBB1_5")
    assert run(kernel(F_NEW, 1), swapped)[0] == 1


def test_a_rename_and_a_removal_are_reported_as_such():
    old = kernel(F_OLD, 0) + kernel(G, 1)
    new = kernel(F_NEW, 0)
    rename = (r"<(\d+), false, true, ", r"<\1, false, ") if FILT else (r"ILi1ELb0ELb1E", "ILi1ELb0E")
    # without the rename: two kernels gone, one new, nothing to compare
    assert kid.compare(old, new) == (sorted([shown(F_OLD), shown(G)]), [shown(F_NEW)], [], 0)
    assert run(old, new)[0] == 1
    # with it: f is the same kernel under its new name, g is removed
    assert kid.compare(old, new, rename) == ([shown(G)], [], [], 1)
    status, text = run(old, new, rename=rename)
    assert status == 1 and "removed (NOT expected): " + shown(G) in text
    status, text = run(old, new, rename=rename, expect_removed=[shown(G)])
    assert status == 0 and "removed: " + shown(G) in text
    # an expectation that does not come true fails too, and so does an added kernel nobody announced
    assert run(old, new, rename=rename, expect_removed=[shown(G), "h()"])[0] == 1
    assert run(new, old, expect_added=[shown(G)])[0] == 1
    assert run(new, old, expect_added=[shown(G), shown(F_OLD)], expect_removed=[shown(F_NEW)])[0] == 0


def test_command_line(tmp_path):
    a, b = tmp_path / "old.s", tmp_path / "new.s"
    a.write_text(kernel(G, 0) + kernel(F_NEW, 1))
    b.write_text(kernel(F_NEW, 0))
    assert kid.main([str(a), str(b)]) == 1
    assert kid.main([str(a), str(b), "--expect-removed", shown(G)]) == 0
