"""Keys of a sample's information dictionary (src/.../active_learning_loop/sample_maker/namespace.py:1-3)."""
CENTRAL_ATOM_INDEX = "central_atom_index"
AXL_STRUCTURE_IN_ORIGINAL_BOX = "axl_structure_in_original_box"
AXL_STRUCTURE_IN_NEW_BOX = "axl_structure_in_new_box"
