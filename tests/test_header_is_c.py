"""CPU: include/kmerhash_amd.h is a plain C header (C99) -- any FFI that speaks C can bind it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles_as_c99_and_links(tmp_path):
    from kmerhash_amd.build import build_library
    build_library()
    src = tmp_path / "use.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  kh_table* t = 0; uint64_t n = 0;\n'
                   '  kh_status s = kh_create(&t, KH_KIND_ROBINHOOD, 8, 4, KH_HASH_MURMUR3_X86_128_LO64, 43, 128, 0.35f, 0.8f, 0);\n'
                   '  if (s == KH_OK) { kh_size(t, &n); kh_destroy(t); }\n'
                   '  printf("%s status=%d\\n", kh_version(), (int)s);\n  return 0;\n}\n')
    exe = tmp_path / "use"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gfx950" in r.stdout     # status is KH_ERR_HIP (5) without a GPU, KH_OK with one


def test_every_environment_switch_is_documented():
    """every KH_* / KHD_* variable the libraries read (getenv in kmerhash_amd/csrc) is listed in INTEGRATION.md's table of switches"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = set()
    for f in ("kmerhash_amd/csrc/kmerhash_amd.hip", "kmerhash_amd/csrc/kmerhash_amd_dist.cpp", "kmerhash_amd/csrc/kh_kernels.h"):
        names |= set(re.findall(r'getenv\("(KHD?_[A-Z0-9_]+)"\)', open(os.path.join(root, f)).read()))
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    missing = sorted(n for n in names if n not in doc)
    assert len(names) >= 15 and not missing, missing


def test_shard_plan_destroy_contract_and_signature(tmp_path):
    """kh_shard_plan_destroy keeps its signature (void, one plan pointer: a C function pointer of that type takes it, -Werror) and the
    header states when it may be called: once the last permute has returned, the block going back to the pool behind the queued work"""
    import re
    hdr = open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read()
    assert len(re.findall(r"^void\s+kh_shard_plan_destroy\s*\(\s*kh_shard_plan\s*\*\s*plan\s*\)\s*;", hdr, flags=re.M)) == 1
    # the comment that ends right above the declaration is the contract
    doc = re.search(r"/\*((?:(?!\*/).)*)\*/\s*void\s+kh_shard_plan_destroy", hdr, flags=re.S)
    assert doc, "kh_shard_plan_destroy has no contract comment"
    text = " ".join(doc.group(1).replace("*", " ").split())
    for phrase in ("as soon as the last kh_shard_plan_permute / _permute_global call has RETURNED",
                   "returns to the library's pool only after every permutation queued from the plan has run",
                   "never permuted", "n == 0", "freed at once"):
        assert phrase in text, phrase
    src = tmp_path / "sig.c"
    src.write_text('#include "kmerhash_amd.h"\n'
                   'typedef void (*destroy_fn)(kh_shard_plan*);\n'
                   'int main(void) { destroy_fn f = kh_shard_plan_destroy; return f == 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sig.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the C++ layer relies on it: find and count destroy their plan with the permutations queued, and add no wait of their own
    dist = open(os.path.join(ROOT, "kmerhash_amd", "csrc", "kmerhash_amd_dist.cpp")).read()
    assert re.search(r"~PlanGuard\(\)\s*\{\s*kh_shard_plan_destroy\(\s*h\s*\)\s*;\s*\}", dist)
