"""Register use of the label pass (assign_kernel, csrc/kmeans.hip) as compiled
for gfx950: no instance uses scratch, and the XL instances that stream up to
32 channels (config 2 runs assign_kernel<32, 64, true, true>) stay within the
128 registers that four waves per SIMD allow."""
import os
import re
import subprocess


def test_no_assign_kernel_spills_and_xl_keeps_its_occupancy(tmp_path):
    from milwrm_amd import build as B

    src = os.path.join(B.CSRC, "kmeans.hip")
    cmd = [B.HIPCC] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                  str(tmp_path / "kmeans.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    agprs = [int(x) for x in re.findall(r" AGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(agprs)
    inst = {}
    for n, s, v, a in zip(names, scratch, vgprs, agprs):
        m = re.search(r"assign_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])EEEv", n)
        if m:  # (CMAX, KS, SC, XL)
            inst[tuple(int(x) for x in m.groups())] = (s, v + a)
    # every instance the launch code can pick: CMAX 8 / 16 / 32 / 64 x KS x SC, XL from CMAX 32, CMAX 52 for XL
    want = {(cm, ks, sc, 0) for cm in (8, 16, 32, 64) for ks in (64, 128) for sc in (0, 1)}
    want |= {(cm, ks, 1, 1) for cm in (32, 64) for ks in (64, 128)} | {(52, 64, 1, 1)}
    assert want <= set(inst), sorted(want - set(inst))
    assert not any(s for s, _ in inst.values()), {i: s for i, (s, _) in inst.items() if s}
    # XL: the wave's LDS tile is 64 * C floats, 4 waves per block.  Up to 32
    # channels LDS leaves room for 4 blocks per CU, so 128 registers; the
    # 52- and 64-channel forms never had that (149 / 168 registers before the
    # skip) and are held to what their LDS allows: 3 blocks at C <= 52 (168
    # registers), 2 blocks from C = 53 (256)
    cap = {32: 128, 52: 168, 64: 256}
    xl = {i: regs for i, (_, regs) in inst.items() if i[3] == 1}
    assert all(regs <= cap[i[0]] for i, regs in xl.items()), xl
