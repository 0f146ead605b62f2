"""The sampling side of the reference's active-learning loop: atom selectors, environment excisors and the four sample makers
(noop, excise_and_noop, excise_and_repaint on the repaint generator, excise_and_random) with their factory
(src/.../active_learning_loop/)."""
