"""The part of the reference's active-learning loop that stands on the repaint generator: atom selectors, environment excisors
and the excise-and-repaint sample maker (src/.../active_learning_loop/)."""
