"""Sample makers: new candidate structures around the uncertain atoms of a frame."""
