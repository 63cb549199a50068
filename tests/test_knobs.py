"""Every GALAHGPU_* name that the tests, the scripts, the header and the
documents speak of is one the library reads: a knob that was removed from
galah_amd/ must leave them too (a test that sets a dead knob compares the
default path with itself)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKEN = re.compile(r"GALAHGPU_[A-Z0-9_]+")
# not the library's: the header's include guard, and the directory that
# rust/galah-gpu-sys/build.rs links from
EXEMPT = {"GALAHGPU_H", "GALAHGPU_LIB_DIR"}


def read(path):
    with open(path, "rb") as f:
        return f.read().decode("utf-8", "replace")


def files(pattern):
    return [p for p in sorted(glob.glob(os.path.join(ROOT, pattern))) if os.path.isfile(p)]


def design_section_7():
    text = read(os.path.join(ROOT, "DESIGN.md"))
    start = text.index("\n## 7. ")
    end = text.find("\n## ", start + 1)
    return text[start:end if end >= 0 else len(text)]


def test_every_knob_named_outside_the_library_is_read_by_it():
    library = "".join(read(p) for p in files("galah_amd/csrc/*") + [os.path.join(ROOT, "galah_amd", "__init__.py")])
    named = {}
    for pattern in ("tests/*.py", "scripts/*", "INTEGRATION.md", "include/*"):
        for p in files(pattern):
            for t in TOKEN.findall(read(p)):
                named.setdefault(t, os.path.relpath(p, ROOT))
    for t in TOKEN.findall(design_section_7()):
        named.setdefault(t, "DESIGN.md section 7")
    assert len(named) > 20  # (the patterns found the files)
    dead = {t: where for t, where in named.items() if t not in EXEMPT and t not in library}
    assert not dead, "named but read nowhere in galah_amd/: %s" % dead
