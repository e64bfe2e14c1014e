"""The decisions of a launch-group capture (safevla_amd/csrc/launch_group.h) without HIP: tests/helpers/launch_group_cases.cpp drives captures whose flush functions
print instead of launching, compiled with a plain host compiler.  The expected lines are written out from the rules of the header: a member's launches keep their
call order (pending ones go ahead of a launch that cannot be deferred and of a deferral into a full queue), one stream per capture, every deferred launch counted once."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# "grouped a b c" / "single a": one issue through a flush function; "direct x": a launch that could not be deferred was let through; "ending": svla_group_end is called next
EXPECTED = """
case 1
ending
grouped m0.a m1.a m2.a
grouped m0.b m1.b m2.b
end 0
stats 2 0
case 2
ending
grouped m0.a m1.a m2.a
single m0.b
single m1.b
single m2.b
end 0
stats 1 3
case 3
ending
single m0.a
single m0.b
single m1.a
single m2.a
single m2.b
end 0
stats 0 5
case 4
single m1.a
direct m1.x
ending
single m0.a
single m1.b
single m2.a
end 0
stats 0 4
case 5
direct m0.x
direct m1.x
direct m2.x
ending
grouped m0.a m1.a m2.a
end 0
stats 1 0
case 6
single m0.l0
single m0.l1
single m0.l2
single m0.l3
single m0.l4
single m0.l5
single m0.l6
single m0.l7
ending
single m0.l8
end 0
stats 0 9
case 7
refused m0.b -1
refused m0.x -1
ending
end -1
stats 0 0
begin 0
ending
end 0
stats 0 0
case 8
protocol -1 -1 -1 0 -1 -1 -1 0 0
stats 0 0
"""


def test_capture_logic_with_recording_flush_functions(tmp_path):
    """1: three members in lockstep, two grouped issues; 2: grids differ at the second launch; 3: unequal launch counts; 4: a launch that cannot be deferred behind a
    deferred one; 5: in front of one (the assembly main launch and its row tail); 6: SVLA_MAXQ + 1 deferrals of one member; 7: another stream at a site and at the
    end, then a capture that works and an empty one ended on NULL; 8: the protocol errors (nothing open, members out of range, nesting, member out of range)"""
    from safevla_amd import build
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or os.path.join(os.path.dirname(build.CLANG), "clang++")
    exe = str(tmp_path / "launch_group_cases")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "safevla_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "launch_group_cases.cpp"),
                    "-o", exe], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert got == EXPECTED.strip().splitlines()
