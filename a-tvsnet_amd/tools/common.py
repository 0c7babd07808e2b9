"""Console prefixes used by the entry point (reference: tools/common.py:15-51); write_json, the tools' one report writer."""
import json
import os
import time


def write_json(path, report):
    """A tool's report into `path` (its folder is made): keys sorted, one space of indent, a closing newline."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write('\n')


class _Notify(object):
    ENDC = '\033[0m'

    def _stamp(self, colour, tag):
        return '%s[%s %s]' % (colour, tag, time.strftime('%H:%M:%S'))

    @property
    def INFO(self):
        return self._stamp('\033[94m', 'INFO')

    @property
    def WARNING(self):
        return self._stamp('\033[93m', 'WARNING')

    @property
    def FAIL(self):
        return self._stamp('\033[91m', 'ERROR')


Notify = _Notify()
