"""Generate tests/golden/workspace_surface.json from the reference's workspace file.

    python tests/golden/make_workspace_surface.py <reference>/workspaces/CorrelatedPhotonMappingSingleVolume.inv

For every processor the workspace instantiates (org.inviwo.* types, in the file's order): its class identifier and the port
and property identifiers it serialises -- what tests/test_modules.py holds the processor factory to.  Identifiers only.
"""
import json
import re
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent / "workspace_surface.json"


def main(inv):
    text = Path(inv).read_text(errors="ignore")
    processors = []
    for m in re.finditer(r'<Processor type="(org\.inviwo\.[A-Za-z0-9]+)"(.*?)</Processor>', text, flags=re.S):
        cid, body = m.group(1), m.group(2)
        processors.append({"type": cid, **{kind: re.findall(r'<%s type="[^"]*" identifier="([^"]+)"' % kind, body)
                                           for kind in ("InPort", "OutPort", "Property")}})
    used = sorted(set(re.findall(r'<Processor type="(org\.inviwo\.[A-Za-z0-9]+)"', text)))
    OUT.write_text(json.dumps({"workspace": Path(inv).name, "processor_types": used, "processors": processors}, indent=1) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
