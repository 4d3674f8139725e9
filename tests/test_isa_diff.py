"""tools/isa_diff.py on hand-written assembly: label renumbering and comments do not count,
an instruction or a descriptor field does, renamed kernels are matched through the map."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernel(name, idx, body, vgpr=8, note=""):
    return f"""\t.globl\t{name}
{name}:
\ts_load_dword s0, s[4:5], 0x0 ; {note}
{body}
.LBB{idx}_1: ; %loop {note}
\ts_cbranch_scc1 .LBB{idx}_1
\ts_endpgm
.Lfunc_end{idx}:
\t.section\t.rodata
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t.end_amdhsa_kernel
\t.text
"""


def _run(tmp_path, old, new, *args):
    a, b = tmp_path / "old.s", tmp_path / "new.s"
    a.write_text(old)
    b.write_text(new)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_diff.py"), str(a), str(b), *args],
                       capture_output=True, text=True)
    return r.returncode, r.stdout


def test_removed_kernel_renumbers_labels_without_a_difference(tmp_path):
    add = "\tv_add_f32 v0, v0, v1"
    old = _kernel("k_dead", 0, add) + _kernel("k_live", 1, add, note="old build")
    new = _kernel("k_live", 0, add, note="new build")
    rc, out = _run(tmp_path, old, new)
    assert rc == 0 and "differing 0, added 0, removed 1" in out and "removed: k_dead" in out, out


def test_instruction_and_descriptor_changes_are_reported(tmp_path):
    old = _kernel("k_a", 0, "\tv_add_f32 v0, v0, v1") + _kernel("k_b", 1, "\tv_mul_f32 v0, v0, v1")
    new = _kernel("k_a", 0, "\tv_sub_f32 v0, v0, v1") + _kernel("k_b", 1, "\tv_mul_f32 v0, v0, v1", vgpr=9)
    rc, out = _run(tmp_path, old, new)
    assert rc == 1 and "differs (text): k_a" in out and "differs (descriptor): k_b" in out, out


def test_rename_map_and_added_kernel(tmp_path):
    add = "\tv_add_f32 v0, v0, v1"
    old, new = _kernel("k_tILb0EE", 0, add), _kernel("k_t", 0, add)
    rc, out = _run(tmp_path, old, new)
    assert rc == 1 and "added: k_t" in out and "removed: k_tILb0EE" in out, out
    m = tmp_path / "names.txt"
    m.write_text("k_tILb0EE k_t\n")
    rc, out = _run(tmp_path, old, new, "--map", str(m))
    assert rc == 0 and "common 1, renames applied 1, differing 0, added 0, removed 0" in out, out
