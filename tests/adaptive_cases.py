"""The free-lattice adaptive-corrector cases of tests/golden/make_golden_adaptive.py, in the form of cases.ADAPTIVE."""
import cases
import nets

FREE_LATTICE = {
    "traj_adaptive_free_lattice": (cases.noise_ns(10, sigma_min=1e-3, sigma_max=0.2, schedule_type="linear"),
                                   dict(cases.sampling_ns(8, 1, M=2, fixed=False), algorithm="adaptive_corrector"),
                                   lambda eb: nets.mlp_net(8, 1)),
    "traj_adaptive_fake_free_lattice": (cases.noise_ns(8, corrector_r=0.5),
                                        dict(cases.sampling_ns(8, 2, M=2, fixed=False), algorithm="adaptive_corrector"), None),
}

# every adaptive fixture: the two fixed-lattice ones of make_golden.py and the free-lattice ones
ALL = dict(cases.ADAPTIVE, **FREE_LATTICE)
