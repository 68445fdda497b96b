"""``python -m emavfi IN.y4m OUT.y4m`` (emavfi.cli)."""
import sys

from .cli import main

sys.exit(main())
