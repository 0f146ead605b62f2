"""Generate tests/golden/stillinger_weber/lammps_si8_frames.npz from the LAMMPS record in the reference tree (container-only).

    python tests/golden/make_golden_stillinger_weber.py <the reference checkout>

configuration_templates/mtp/mtp_example/dump.si-300-1.yaml holds the box, the positions and the forces LAMMPS wrote for 11 MD
frames of 8-atom Si in a 5.43 A box under `pair_style sw` with Si.sw, thermo_log.yaml the PotEng of the same steps.  Data only:
nothing of the reference is imported.  (The coefficient files beside the fixture are copies of the reference's
data/stillinger_weber_coefficients/Si.sw and SiGe.sw.)

  box      [F,3]    box sides (Angstrom), the lower bounds are zero
  x        [F,8,3]  positions, atoms in id order
  f        [F,8,3]  forces (eV / Angstrom)
  pot_eng  [F]      PotEng (eV)
  step     [F]      time step of the frame
"""
import os
import sys

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("MDX_GOLDEN_OUT", os.path.join(HERE, "stillinger_weber"))
EXAMPLE = os.path.join("configuration_templates", "mtp", "mtp_example")


def golden_stillinger_weber(reference):
    with open(os.path.join(reference, EXAMPLE, "dump.si-300-1.yaml")) as fd:
        frames = list(yaml.safe_load_all(fd))
    with open(os.path.join(reference, EXAMPLE, "thermo_log.yaml")) as fd:
        thermo = yaml.safe_load(fd)
    pot_eng = {int(row[0]): float(row[thermo["keywords"].index("PotEng")]) for row in thermo["data"]}
    box, x, f, step = [], [], [], []
    for frame in frames:
        assert all(float(lo) == 0.0 for lo, _ in frame["box"]) and frame["natoms"] == 8
        column = {name: k for k, name in enumerate(frame["keywords"])}
        rows = sorted(frame["data"], key=lambda row: row[column["id"]])
        assert all(row[column["type"]] == 1 for row in rows)
        box.append([float(hi) for _, hi in frame["box"]])
        x.append([[float(row[column[c]]) for c in ("x", "y", "z")] for row in rows])
        f.append([[float(row[column[c]]) for c in ("fx", "fy", "fz")] for row in rows])
        step.append(int(frame["timestep"]))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "lammps_si8_frames.npz")
    np.savez_compressed(path, box=np.array(box), x=np.array(x), f=np.array(f), pot_eng=np.array([pot_eng[s] for s in step]),
                        step=np.array(step, dtype=np.int64))
    print(f"wrote lammps_si8_frames.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    golden_stillinger_weber(sys.argv[1])
