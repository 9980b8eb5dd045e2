"""Generate tests/golden/detect_metrics.json: LoRaDetector<float>::detect of the reference
(include/lora_phy/LoRaDetector.hpp with include/lora_phy/kissfft.hh, compiled from the
reference checkout's include path) on the seeded windows of tests/detect_checker.py
golden_windows().

Per window the file records the SF, the window's name and sha256 (the tests regenerate the
same input and check it), detect()'s return value and the fp32 bit patterns of power,
powerAvg and fIndex.  The driver below is ours; it is compiled into a temporary directory
and nothing of the reference, in source or compiled form, is kept.

Run where the reference checkout exists: python tests/golden/make_detect_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = os.environ.get("LORA_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "detect_metrics.json")

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include <lora_phy/LoRaDetector.hpp>
static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }
int main(int argc, char** argv) {  // argv[1]: N, stdin: windows of N complex<float>
  const size_t N = std::strtoul(argv[1], nullptr, 10);
  std::vector<std::complex<float>> in(N), out(N), w(N);
  static kissfft_plan<float> plan;
  kissfft<float>::init(plan, (int)N, false);
  kissfft<float> fft(plan);
  LoRaDetector<float> det(N, in.data(), out.data(), fft);
  while (std::fread(w.data(), sizeof(w[0]), N, stdin) == N) {
    for (size_t i = 0; i < N; ++i) det.feed(i, w[i]);
    float p, pav, fi;
    const size_t idx = det.detect(p, pav, fi);
    std::printf("%zu %u %u %u\n", idx, bits(p), bits(pav), bits(fi));
  }
  return 0;
}
"""


def main():
    if not os.path.isdir(os.path.join(REF, "include", "lora_phy")):
        sys.exit(f"the reference checkout is not at {REF}")
    from tests.detect_checker import GOLDEN_SFS, golden_windows
    from tests.golden_inputs import sha
    from oracle.pyoracle import Oracle

    M = Oracle()
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "detect_driver.cpp"), os.path.join(tmp, "detect_driver")
        with open(src, "w") as fh:
            fh.write(DRIVER)
        # the reference's own flags (CMakeLists.txt:4-7: C++11, -O2)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(REF, "include"), "-o", exe, src])
        for sf in GOLDEN_SFS:
            wins = golden_windows(M, sf)
            blob = b"".join(w.tobytes() for _, w in wins)
            lines = subprocess.run([exe, str(1 << sf)], input=blob, capture_output=True, check=True).stdout.split(b"\n")
            for (name, w), line in zip(wins, lines):
                idx, p, pav, fi = (int(t) for t in line.split())
                records.append({"sf": sf, "name": name, "sha256": sha(w), "index": idx, "power": p,
                                "power_avg": pav, "f_index": fi})
            assert len([ln for ln in lines if ln]) == len(wins)
    with open(OUT, "w") as fh:
        json.dump({"note": "LoRaDetector<float>::detect of the reference on detect_checker.golden_windows(); "
                           "floats as fp32 bit patterns", "records": records}, fh, indent=0)
    print(f"{len(records)} records -> {OUT} ({os.path.getsize(OUT)} bytes)")
    for r in records:
        if r["sf"] == 7:
            print(r["name"], r["index"], *(np.uint32(r[k]).view(np.float32) for k in ("power", "power_avg", "f_index")))


if __name__ == "__main__":
    main()
