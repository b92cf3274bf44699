"""The name tests/test_{param_fields,hyperelastic,hosford}_build.py import the build-check helpers by; they live in
tools/check_device_asm.py, which is also the command-line tool."""
from check_device_asm import *  # noqa: F401,F403
