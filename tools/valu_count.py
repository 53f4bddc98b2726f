#!/usr/bin/env python3
"""Static instruction counts of the hot kernels from the gfx950 assembly (hipcc -S): VALU / LDS / VMEM per wave and VALU
per output dword (the unrolled row loop is straight-line code; a thread writes rows_per_thread x 4 output dwords).
    python tools/valu_count.py > profiles/<tag>_valu_counts.txt          (build container, no GPU needed)
    python tools/valu_count.py --bilateral      the window-row loop of blur_bilateral_tiled_kernel<3, RC>: VALU and ds_read
                                                per output byte and window row, and per tap of the class's 2 RC + 1 columns
    python tools/valu_count.py --conv           the window-row loop of blur_conv_tiled_kernel<C, RC, NT>: the same counts per tap
                                                (NT = 2, the magnitude mode, multiplies every window byte by two taps), and the
                                                scratch, LDS and register sizes of every instantiation"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "heterogeneous-opencl-image-processing-engine_amd", "csrc", "blur_kernels.hip")


def main():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, SRC],
                       check=True, stderr=subprocess.DEVNULL)
        text = open(out).read().splitlines()
    want = {
        "3x3 tiled, rows/thread 8 (split-then-shift row pass: shipped)": "_ZN7mi_blur17blur_tiled_kernelILi3ELi1ELi8ELb1ELb0ELb0EEEvNS_11TiledParamsE",
        "3x3 tiled, rows/thread 8 (raw-window row pass: A/B form)": "_ZN7mi_blur19blur_tiled_x_kernelILi3ELi1ELi8ELi1EEEvNS_11TiledParamsE",
        "3x3 fused stream, rows/thread 8": "_ZN7mi_blur17blur_fused_kernelILi3ELi1ELi8EEEvNS_11TiledParamsENS_11FusedParamsE",
        "3x3 fused stream with dynamic tail, rows/thread 8": "_ZN7mi_blur22blur_fused_tail_kernelILi3ELi1ELi8ELb0EEEvNS_11TiledParamsENS_11FusedParamsE",
        "5x5 tiled, rows/thread 8 (raw-window row pass: shipped)": "_ZN7mi_blur17blur_tiled_kernelILi3ELi2ELi8ELb1ELb0ELb0EEEvNS_11TiledParamsE",
        "5x5 tiled, rows/thread 8 (split-then-shift row pass: round-1 form)": "_ZN7mi_blur19blur_tiled_x_kernelILi3ELi2ELi8ELi0EEEvNS_11TiledParamsE",
        "5x5 streaming variant": "_ZN7mi_blur18blur_stream_kernelILi3ELi2EEEvNS_12StreamParamsE",
        "3x3 direct (LDS-free), 8 rows per lane": "_ZN7mi_blur18blur_direct_kernelILi3ELi1ELi8EEEvNS_12DirectParamsE",
        "5x5 direct (LDS-free), 8 rows per lane": "_ZN7mi_blur18blur_direct_kernelILi3ELi2ELi8EEEvNS_12DirectParamsE",
    }
    print("static counts per wave, gfx950, hipcc -O3 (C = 3); VALU per output dword = VALU / (8 rows x 4 dwords)")
    for label, sym in want.items():
        try:
            a = next(i for i, l in enumerate(text) if l.startswith(sym + ":"))
        except StopIteration:
            print(f"{label}: symbol not found"); continue
        b = next(i for i in range(a, len(text)) if text[i].startswith(".Lfunc_end"))
        body = text[a:b]
        ops = [l.split()[0] for l in body if re.match(r"^\s+[a-z]", l) and not l.strip().startswith((".", ";"))]
        valu = sum(o.startswith("v_") for o in ops)
        c = lambda p: sum(o.startswith(p) for o in ops)
        per = f"{valu / 32:.1f}" if "streaming" not in label else "n/a (loop)"
        print(f"{label:70s} VALU {valu:5d} ({per} per output dword)  v_perm {c('v_perm'):4d}  v_alignbit {c('v_alignbit'):4d}  v_and {c('v_and_b32'):4d}  "
              f"v_pk_mad {c('v_pk_mad'):4d}  ds_read {c('ds_read'):3d}  vmem {c('global_') + c('buffer_'):3d}  s_waitcnt {c('s_waitcnt'):3d}")


def bilateral():
    src = os.path.join(os.path.dirname(SRC), "bilateral_kernels.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, src],
                       check=True, stderr=subprocess.DEVNULL)
        text = open(out).read().splitlines()
    print("blur_bilateral_tiled_kernel<C, RC>, gfx950, hipcc -O3: the window-row loop (one pass = one window row of one output dword = 4 output bytes)")
    for ch in (1, 3, 4):
        for rc in (2, 4, 8):
            sym = f"_ZN7mi_blur12_GLOBAL__N_127blur_bilateral_tiled_kernelILi{ch}ELi{rc}EEEvNS0_14BilTiledParamsIXT0_EEE"
            a = next(i for i, l in enumerate(text) if l.startswith(sym + ":"))
            b = next(i for i in range(a, len(text)) if text[i].startswith(".Lfunc_end"))
            la = next(i for i in range(a, b) if "Inner Loop Header: Depth=2" in text[i])
            lb = next(i for i in range(la, b) if "s_cbranch" in text[i])
            ops = [l.split()[0] for l in text[la:lb + 1] if re.match(r"^\s+[a-z]", l)]
            valu, ds, gather = sum(o.startswith("v_") for o in ops), sum(o.startswith("ds_read") for o in ops), sum(o == "ds_read_u8" for o in ops)
            cols = 2 * rc + 1
            print(f"C={ch} RC={rc}: per row pass VALU {valu:4d}  ds_read {ds:3d} (of them ds_read_u8 {gather:3d})  s_waitcnt {sum(o == 's_waitcnt' for o in ops):2d}"
                  f"   per output byte and row: VALU {valu / 4:6.1f}  ds_read {ds / 4:5.1f}   per tap of the {cols} columns: VALU {valu / 4 / cols:4.2f}  ds_read {ds / 4 / cols:4.2f}")


def conv():
    src = os.path.join(os.path.dirname(SRC), "conv_kernels.hip")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, src],
                       check=True, stderr=subprocess.DEVNULL)
        text = open(out).read().splitlines()
    print("blur_conv_tiled_kernel<C, RC, NT>, gfx950, hipcc -O3: the window-row loop (one pass = one window row of one output dword = 4 output bytes)")
    for ch in (1, 3, 4):
        for rc in (1, 2, 3, 5, 7):
            for nt in (1, 2):
                sym = f"_ZN7mi_blur12_GLOBAL__N_122blur_conv_tiled_kernelILi{ch}ELi{rc}ELi{nt}EEEvNS0_15ConvTiledParamsIXT0_EXT1_EEE"
                a = next(i for i, l in enumerate(text) if l.startswith(sym + ":"))
                b = next(i for i in range(a, len(text)) if text[i].startswith(".Lfunc_end"))
                la = next(i for i in range(a, b) if "Inner Loop Header: Depth=2" in text[i])
                lb = next(i for i in range(la, b) if "s_cbranch" in text[i])
                ops = [l.split()[0] for l in text[la:lb + 1] if re.match(r"^\s+[a-z]", l)]
                valu, ds, salu = sum(o.startswith("v_") for o in ops), sum(o.startswith("ds_read") for o in ops), sum(o.startswith("s_") for o in ops)
                mads = sum(o.startswith(("v_mad_i32_i24", "v_mul_i32_i24", "v_mad_u32_u24", "v_mul_u32_u24")) for o in ops)
                rows = mads / (4.0 * (2 * rc + 1) * nt)               # the compiler may unroll the row loop: window rows per pass
                print(f"C={ch} RC={rc} NT={nt}: per loop pass ({rows:3.1f} window rows) VALU {valu:4d} (24-bit mul/mad {mads:4d})  SALU {salu:3d}  ds_read {ds:2d}  s_waitcnt {sum(o == 's_waitcnt' for o in ops):2d}"
                      f"   per tap (one multiply of one output byte): VALU {valu / mads:4.2f}  ds_read {ds / mads:5.3f}")
    print("every blur_conv_* kernel: .amdhsa_private_segment_fixed_size (scratch bytes), static LDS bytes, VGPRs, SGPRs")
    worst = 0
    for i, l in enumerate(text):
        m = re.match(r"\s*\.amdhsa_kernel (\S*blur_conv\S*)", l)
        if not m:
            continue
        e = next(j for j in range(i, len(text)) if ".end_amdhsa_kernel" in text[j])
        get = lambda key: int(next(re.search(key + r" (\d+)", t).group(1) for t in text[i:e] if key in t))
        scratch = get(".amdhsa_private_segment_fixed_size")
        worst = max(worst, scratch)
        short = re.sub(r".*(blur_conv_(?:tiled|generic)_kernel)(?:ILi(\d)ELi(\d)ELi(\d)E)?.*", lambda q: q.group(1) + (f"<{q.group(2)},{q.group(3)},{q.group(4)}>" if q.group(2) else ""), m.group(1))
        print(f"  {short:34s} scratch {scratch:3d}  lds {get('.amdhsa_group_segment_fixed_size'):5d}  vgpr {get('.amdhsa_next_free_vgpr'):3d}  sgpr {get('.amdhsa_next_free_sgpr'):3d}")
    print(f"largest scratch size: {worst} bytes")


if __name__ == "__main__":
    a = sys.argv[1:]
    conv() if "--conv" in a else bilateral() if "--bilateral" in a else main()
