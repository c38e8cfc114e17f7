"""CPU tier: the pin list of the GPT-2 model handle (lmrl-gym_amd/csrc/prefix_pins.h — pin, unpin, destroy with pins alive, a null pin) as a
stand-alone host program with the forward stubbed out, under AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pin_list_under_sanitizers():
    src = os.path.join(ROOT, "tests", "prefix_pins_harness.cpp")
    exe = os.path.join(ROOT, "tests", "_build", "prefix_pins_harness")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
