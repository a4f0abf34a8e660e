"""Command lines over the package's objects (the reference's scripts under demos / experiments)."""
