"""Environment excisors: the atoms around a central atom, cut out of a frame by ONE launch of mdx_excise_environments."""
