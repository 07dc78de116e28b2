#!/usr/bin/env python3
"""Per-kernel register / LDS / scratch use of a built libdfgnn.so (from the code object's metadata notes).
usage: python tools/kernel_resources.py [pattern] [lib] [--check]
pattern: a regular expression over the mangled kernel names, e.g. dense, gt_typed, gt_bias_(wave|group), gt_tbias, gatv2_edge, gt_gate.
--check: print a summary line and exit with status 1 if a matched kernel spills or uses scratch (or none matched) -- how
the no-scratch rule of the any-graph pairs (gt_typed, gt_tbias, gatv2_edge) is checked without a GPU."""
import re, subprocess, sys
check = "--check" in sys.argv
sys.argv = [a for a in sys.argv if a != "--check"]
pat = sys.argv[1] if len(sys.argv) > 1 else "dense"
lib = sys.argv[2] if len(sys.argv) > 2 else "df-gnn_amd/libdfgnn_hip.so"
import tempfile, os
tmp = tempfile.mkdtemp()
fb = os.path.join(tmp, "fb")
subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fb], check=True)
blob = open(fb, "rb").read()
magic = b"__CLANG_OFFLOAD_BUNDLE__"
offs = [m.start() for m in re.finditer(magic, blob)] + [len(blob)]
out = ""
for k in range(len(offs) - 1):   # one bundle per translation unit
    part, co = os.path.join(tmp, f"b{k}"), os.path.join(tmp, f"co{k}")
    open(part, "wb").write(blob[offs[k]:offs[k + 1]])
    subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--type=o", "--unbundle", f"--input={part}",
                    f"--output={co}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True, capture_output=True)
    out += subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
seen, bad = 0, []
for blk in out.split("- .agpr_count:")[1:]:
    name = re.search(r"\.name:\s+(\S+)", blk)
    if not name or not re.search(pat, name.group(1)): continue
    g = lambda k: (re.search(rf"\.{k}:\s+(\d+)", blk) or [0, "?"])[1]
    dem = subprocess.run(["c++filt", name.group(1)], capture_output=True, text=True).stdout.strip()
    seen += 1
    if g("vgpr_spill_count") != "0" or g("private_segment_fixed_size") != "0": bad.append(dem)
    print(f"vgpr {g('vgpr_count'):>3} agpr {blk.split()[0]:>3} sgpr {g('sgpr_count'):>3} spill {g('vgpr_spill_count'):>3} "
          f"scratch {g('private_segment_fixed_size'):>5} lds {g('group_segment_fixed_size'):>6}  {dem[:110]}")
if check:
    print(f"{seen} kernels match {pat!r}; {len(bad)} spill or use scratch")
    sys.exit(1 if bad or not seen else 0)
