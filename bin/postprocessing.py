#!/usr/bin/python3
"""Drop-in `postprocessing.py` for PYP (link or copy it to $PYP_DIR/external/postprocessing/postprocessing.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.realpath(__file__)), ".."))
from pyp_amd.surface import warm  # noqa: E402

warm.start(pinned=0)      # GPU context creation overlaps the imports and the reading of the maps
from pyp_amd.surface import cli  # noqa: E402

sys.exit(cli.postprocessing_main())
