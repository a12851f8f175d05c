"""
Sinks: where a decoded signal goes.  Three small host-only classes with the constructors of the reference package's ``sink``
module -- ``wavFile(filename, sig)``, ``image(filename, mat)``, ``csv(filename, data, titles=None)``.  As there, ``write`` (and
``show`` on ``image``) is a property: reading it does the work and hands the object back, so ``sink.wavFile(p, audio).write``
is a whole statement.

Nothing here launches a kernel.  A ``commSignal`` whose samples live on the device is downloaded by its ``signal`` property,
which keeps the host copy; ``wavFile`` reads it once.  SciPy's WAV writer and PIL are imported where they are used, so importing
the package needs neither.
"""
import itertools


class wavFile:
    """A WAV file made of a signal's samples at its sample rate (scipy.io.wavfile decides the sample format from the dtype)."""

    def __init__(self, filename, sig):
        """filename: path of the file to write; sig: anything with ``sampRate`` and ``signal``, such as a ``commSignal``"""
        self._path = filename
        self._source = sig

    @property
    def write(self):
        """writes the file; returns this object"""
        from scipy.io import wavfile
        rate, samples = self._source.sampRate, self._source.signal       # one read: a device-resident signal comes down here
        wavfile.write(self._path, rate, samples)
        return self


class image:
    """A picture made of a matrix of pixel values (rows x columns, or rows x columns x channels), to save or to look at."""

    def __init__(self, filename, mat):
        """filename: path of the file ``write`` saves to, the extension choosing the format; mat: the pixel array"""
        from PIL import Image
        self._path = filename
        self._picture = Image.fromarray(mat)

    @property
    def write(self):
        """saves the picture; returns this object"""
        self._picture.save(self._path)
        return self

    @property
    def show(self):
        """opens the picture in the system's viewer; returns this object"""
        self._picture.show()
        return self


class csv:
    """A table written column-wise: ``data`` is a list of columns, ``titles`` an optional heading per column.  Every cell, the
    last of a line included, is followed by a comma, and a column that ends early leaves empty cells (the format
    tests/golden/sink_csv.txt records)."""

    def __init__(self, filename, data, titles=None):
        """filename: path of the file to write; data: the columns, possibly of unequal length; titles: the heading line or None"""
        self._path = filename
        self._columns = data
        self._titles = titles

    @staticmethod
    def _line(cells):
        return "".join("%s," % (cell,) for cell in cells) + "\n"

    @property
    def write(self):
        """writes the file; returns this object"""
        lines = [] if self._titles is None else [self._line(self._titles)]
        lines.extend(self._line(row) for row in itertools.zip_longest(*self._columns, fillvalue=""))
        with open(self._path, "w") as f:
            f.writelines(lines)
        return self
