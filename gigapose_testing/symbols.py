"""What a shared library exports, for the tests that hold a library to its header."""
import subprocess


def exported_symbols(path):
    """The defined dynamic symbols of the library at `path` (text, data, bss and weak), sorted."""
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TDBW")
