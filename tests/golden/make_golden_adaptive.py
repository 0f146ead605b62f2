"""Generate the free-lattice adaptive-corrector fixtures by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_adaptive.py

The reference's own AdaptiveCorrectorGenerator (generators/adaptive_corrector.py:17-148) with use_fixed_lattice_parameters=False:
the two adaptive fixtures of make_golden.py::golden_next have a fixed lattice, so the lattice step size (:108-120 of this
package's generator: computed from one lattice draw, applied with the next) had no reference evidence.  The stubs, the echo
network, the MLP template, the generator builder, the draw recorder and the writer are make_golden.py's, imported unchanged.

  traj_adaptive_free_lattice        MLP template _mlp(8, 1), T 10, M 2, linear schedule sigma 1e-3 .. 0.2, B 5, seed 42
  traj_adaptive_fake_free_lattice   echo network, T 8, M 2, two atom types, corrector_r 0.5, B 4, seed 41 (the settings of
                                    traj_adaptive_fake with a free lattice): a small second case with an exact forward
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)

from diffusion_for_multi_scale_molecular_dynamics.generators.adaptive_corrector import AdaptiveCorrectorGenerator  # noqa: E402


def golden_adaptive_free_lattice():
    for name, kw, netf, B, seed in [
        ("traj_adaptive_free_lattice", dict(T=10, N=8, num_atom_types=1, M=2, fixed=False,
                                            noise_kw=dict(sigma_min=1e-3, sigma_max=0.2, schedule_type="linear")),
         lambda: mg._mlp(8, 1), 5, 42),
        ("traj_adaptive_fake_free_lattice", dict(T=8, N=8, num_atom_types=2, M=2, fixed=False,
                                                 noise_kw=dict(corrector_r=0.5)), None, 4, 41),
    ]:
        net = netf() if netf else None
        gen0, npar, spar = mg.make_generator(record=True, net=net, **kw)
        spar.algorithm = "adaptive_corrector"
        gen = AdaptiveCorrectorGenerator(noise_parameters=npar, sampling_parameters=spar, axl_network=gen0.axl_network)
        torch.manual_seed(seed)
        with torch.no_grad(), mg.DrawRecorder() as rec:
            axl = gen.sample(B, torch.device("cpu"))
        out = dict(final_A=mg._np(axl.A), final_X=mg._np(axl.X), final_L=mg._np(axl.L), batch=np.array(B))
        out.update(rec.pack())
        out.update(mg._pack_records(gen))
        if net is not None:
            out.update(mg._state_dict_np(net))
        mg.save(name + ".npz", **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_adaptive_free_lattice()
