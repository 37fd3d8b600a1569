"""The carver every workspace layout of the library runs on (csrc/car_workspace.h), checked by a stand-alone host program
(tests/host/car_workspace_host.cpp): totals with and without a base agree, every piece is aligned as asked, inside the range and
overlaps no other, a nested layout stays inside its parent's piece, an over-full sub-range is reported and not carved.  Built with g++
alone (the header has no HIP types) and with the address and undefined-behaviour sanitizers, under which the program also writes every
byte of every piece."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "car_workspace_host.cpp")
INC = os.path.join(ROOT, "cross_attention_renderer_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "host", "_build", "car_workspace_host")


def test_the_carver_host_program_passes():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, os.path.join(INC, "car_workspace.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", OUT])
    run = subprocess.run([OUT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "car_workspace: OK" in run.stdout, run.stdout
