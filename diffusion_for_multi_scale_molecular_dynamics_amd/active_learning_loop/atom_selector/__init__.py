"""Which atoms of an uncertain frame become the centres of excised environments (host numpy, as the reference)."""
