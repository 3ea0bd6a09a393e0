"""Kernel metadata of csrc/conv1x1_pair.hip (CPU-only: hipcc cross-compiles).  The kernel keeps both weight matrices of the launch in
registers - 256 of a wave's 512 - and runs one wave per SIMD: a spill would put scratch traffic into the vmcnt stream its
prefetch is waited on with, and more than 512 registers do not exist."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_pair_kernel_fits_one_wave_per_simd_without_scratch(tmp_path):
    import proben_amd  # noqa: F401
    from proben_amd import build
    src = os.path.join(build.CSRC, "conv1x1_pair.hip")
    out = tmp_path / "conv1x1_pair.s"
    cmd = [build.hipcc(), "--offload-arch=" + build.ARCH, "-O3", "-std=c++17", "-x", "hip", "-S", "--cuda-device-only", src, "-o", str(out),
           "-I", os.path.join(ROOT, "include"), "-I", build.CSRC] + build.EXTRA.get("conv1x1_pair.hip", build.EXTRA["default"])
    subprocess.check_call(cmd)
    text = out.read_text()
    bodies = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S)
    assert len(bodies) == 1 and "conv1x1_pair_kernel" in bodies[0][0], [n for n, _ in bodies]
    for name, body in bodies:
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name + ": scratch in use"
        m = re.search(r"\.amdhsa_next_free_vgpr (\d+)", body)
        # 256 registers of weight fragments + accumulators, epilogue values and addresses: 461 today.  The file has 512; the
        # bound leaves the compiler 19 more before this fails and 32 after that before it must spill
        assert m and int(m.group(1)) <= 480, (name, m and m.group(1))
        m = re.search(r"\.amdhsa_accum_offset (\d+)", body)
        assert m and int(m.group(1)) == 256, (name, m and m.group(1))      # all 256 architectural registers, the rest in the accumulation file
        m = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body)
        assert m and int(m.group(1)) == 0, name                            # all LDS is the launch's 160 KiB of dynamic LDS
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
    assert spills and all(int(c) == 0 for c in spills)
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert sizes and all(int(c) == 0 for c in sizes)


def test_pair_entry_point_checks_its_arguments_before_any_device_work():
    """pe_conv1x1_pair_f16 without a GPU: null pointers, channel counts other than the one instantiation, tensors beyond the 32-bit
    buffer offsets and an output that overlaps an input or the other output are refused with a message, before anything touches a device."""
    import __graft_entry__ as g
    g.build()
    import proben_amd
    L = proben_amd._lib.lib()
    err = lambda: L.pe_last_error().decode()
    p = [(i + 1) << 20 for i in range(8)]      # t2, w3, b3, residual, w1_next, b1_next, out, t1_next
    assert L.pe_conv1x1_pair_f16(*p[:7], None, 1, 4, 4, 128, 512, 128, None) != 0 and "null pointer" in err()
    assert L.pe_conv1x1_pair_f16(*p, 0, 4, 4, 128, 512, 128, None) != 0 and "bad dims" in err()
    assert L.pe_conv1x1_pair_f16(*p, 1, 4, 4, 256, 1024, 256, None) != 0 and "128 -> 512 -> 128" in err()
    assert L.pe_conv1x1_pair_f16(*p, 64, 256, 256, 128, 512, 128, None) != 0 and "2 GiB" in err()
    for dst, src, off in ((6, 3, 0), (6, 0, 0), (7, 0, 0), (7, 3, 0), (7, 6, 0), (6, 3, 1024), (7, 3, 16 * 1024 - 2)):
        q = list(p)
        q[dst] = q[src] + off      # an output on, or partly on, an input or the other output (16 pixels: 16 KiB / 4 KiB tensors)
        assert L.pe_conv1x1_pair_f16(*q, 1, 4, 4, 128, 512, 128, None) != 0 and "overlap" in err(), (dst, src, off)
    from proben_amd import layers
    assert layers.conv1x1_pair_supported(128, 512, 128, 32 * 100 * 128) and not layers.conv1x1_pair_supported(256, 1024, 256, 100)
    assert not layers.conv1x1_pair_supported(128, 512, 128, 2 ** 21)      # 2^21 pixels x 1 KiB = 2 GiB
