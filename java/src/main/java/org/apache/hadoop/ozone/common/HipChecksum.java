package org.apache.hadoop.ozone.common;

import java.nio.ByteBuffer;
import java.util.ArrayList;
import java.util.List;

import org.apache.hadoop.hdds.protocol.datanode.proto.ContainerProtos.ChecksumType;
import org.apache.ozone.erasurecode.rawcoder.OzecNative;
import org.apache.ratis.thirdparty.com.google.protobuf.ByteString;
import org.apache.ratis.thirdparty.com.google.protobuf.UnsafeByteOperations;

/**
 * Batch hook of Checksum.computeChecksum(ChunkBuffer) (CM/Checksum.java:157-179): every bytesPerChecksum window of one
 * host buffer checksummed in one libozec call (ozec_checksum_windows / ozec_digest_windows), giving the same
 * ChecksumData the reference's window loop builds -- 4-byte big-endian int2ByteString((int) getValue()) per window, last window short
 * (Checksum.java:59-70).
 *
 * <p>{@link HipChecksumAccelerator} (the provider of hdds-common's ChecksumAccelerator seam,
 * java/patches/hdds-common-checksum-hook.patch) takes this path only when {@link #useGpu} says so: a
 * single-buffer ChunkBuffer, libozec usable, and at least {@code ozone.checksum.hip.batch.min.bytes} bytes.
 * That threshold defaults to never: a host buffer crosses PCIe twice (staging copy, H2D, kernel, D2H) and on MI355X
 * that lost to one core's JDK-class CRC32C at every size measured, 16 KiB to 64 MiB, from 1 and from 16 threads
 * (bench.py --workload stream, checksum_windows_* rows, profiles/r03/).  Every other call runs the reference's own
 * loop unchanged, so the hook never makes Checksum slower.  The GPU CRC is used where the bytes are already on the
 * device (INTEGRATION.md §2).
 *
 * <p>SHA256 / MD5 (MessageDigest per window in the reference, CM/Checksum.java:43-57,76-81) take the same hook through
 * ozec_digest_windows, one GPU lane per window, under a threshold of their own,
 * {@code ozone.checksum.hip.digest.min.bytes}: a core hashes a few hundred MB/s to a few GB/s, far below the host link,
 * so unlike the CRCs a host buffer can pay for the round trip.  The measured crossover is in INTEGRATION.md §2; the
 * default stays never.
 * CM/ = hadoop-hdds/common/src/main/java/org/apache/hadoop/ozone/common/
 */
public final class HipChecksum {
  /** Host buffers of at least this many bytes are checksummed on the GPU (default: none, see above). */
  static final long MIN_GPU_BYTES = Long.getLong("ozone.checksum.hip.batch.min.bytes", Long.MAX_VALUE);

  /** The same for SHA256 / MD5 buffers (default: none; measured crossover in INTEGRATION.md §2). */
  static final long MIN_GPU_DIGEST_BYTES = Long.getLong("ozone.checksum.hip.digest.min.bytes", Long.MAX_VALUE);

  private HipChecksum() {
  }

  /** True when libozec_jni and a GPU are usable. */
  public static boolean isAvailable() {
    return OzecNative.isAvailable();
  }

  /**
   * Whether Checksum.computeChecksum(ChunkBuffer) should take the GPU batch path for this call: only the single-buffer
   * ChunkBuffer (ChunkBufferImplWithByteBuffer, CM/ChunkBufferImplWithByteBuffer.java:78-98), whose iterate() the
   * batch reproduces including the position it leaves; the buffer-list and incremental forms (whose iterate copies
   * across buffers, or rejects a bytesPerChecksum other than its increment) keep the reference's loop.
   */
  public static boolean useGpu(ChecksumType type, ChunkBuffer data) {
    final long min;
    if (type == ChecksumType.CRC32 || type == ChecksumType.CRC32C) {
      min = MIN_GPU_BYTES;
    } else if (type == ChecksumType.SHA256 || type == ChecksumType.MD5) {
      min = MIN_GPU_DIGEST_BYTES;
    } else {
      return false;
    }
    if (min == Long.MAX_VALUE || data.remaining() < min) {
      return false;
    }
    return data instanceof ChunkBufferImplWithByteBuffer && isAvailable();
  }

  /**
   * The ChecksumData of {@code data} (a single-buffer ChunkBuffer, see {@link #useGpu}).  Like the reference's
   * {@code data.iterate(bytesPerChecksum)} loop, it consumes the buffer: its position ends at its limit.
   */
  public static ChecksumData computeChecksum(ChecksumType type, ChunkBuffer data, int bytesPerChecksum) {
    final ByteBuffer b = data.asByteBufferList().get(0);
    final int nativeType = nativeType(type);
    final int each = bytesPerWindow(nativeType);
    final byte[] crcs = computeChecksumBytes(nativeType, b, bytesPerChecksum);
    b.position(b.limit());
    final List<ByteString> list = new ArrayList<>(crcs.length / each);
    for (int i = 0; i < crcs.length; i += each) {
      list.add(UnsafeByteOperations.unsafeWrap(crcs, i, each));
    }
    return new ChecksumData(type, bytesPerChecksum, list);
  }

  private static int nativeType(ChecksumType type) {
    switch (type) {
    case CRC32:
      return OzecNative.CHECKSUM_CRC32;
    case CRC32C:
      return OzecNative.CHECKSUM_CRC32C;
    case SHA256:
      return OzecNative.CHECKSUM_SHA256;
    case MD5:
      return OzecNative.CHECKSUM_MD5;
    default:
      throw new IllegalArgumentException("unsupported checksum type " + type);
    }
  }

  /** Bytes per window: Ints.toByteArray for the CRCs, MessageDigest.getDigestLength() for SHA256 / MD5. */
  static int bytesPerWindow(int type) {
    return type == OzecNative.CHECKSUM_SHA256 ? 32 : type == OzecNative.CHECKSUM_MD5 ? 16 : 4;
  }

  private static boolean isDigest(int type) {
    return type == OzecNative.CHECKSUM_SHA256 || type == OzecNative.CHECKSUM_MD5;
  }

  /**
   * The concatenated window checksums of {@code data} from its position: 4-byte big-endian CRCs
   * (ozec_checksum_windows), or the 32- / 16-byte MessageDigest.digest() of every window (ozec_digest_windows).
   * @param type OzecNative.CHECKSUM_CRC32, CHECKSUM_CRC32C, CHECKSUM_SHA256 or CHECKSUM_MD5
   */
  public static byte[] computeChecksumBytes(int type, ByteBuffer data, int bytesPerChecksum) {
    final int n = data.remaining();
    final int windows = n == 0 ? 0 : (int) ((n + (long) bytesPerChecksum - 1) / bytesPerChecksum);
    final byte[] out = new byte[bytesPerWindow(type) * windows];
    if (n == 0) {
      return out;
    }
    final boolean digest = isDigest(type);
    if (data.isDirect()) {
      if (digest) {
        OzecNative.digestWindowsDirect(type, data, data.position(), n, bytesPerChecksum, out);
      } else {
        OzecNative.checksumWindowsDirect(type, data, data.position(), n, bytesPerChecksum, out);
      }
    } else {
      final byte[] array;
      final int offset;
      if (data.hasArray()) {
        array = data.array();
        offset = data.arrayOffset() + data.position();
      } else {
        array = new byte[n];
        offset = 0;
        data.duplicate().get(array);
      }
      if (digest) {
        OzecNative.digestWindowsArray(type, array, offset, n, bytesPerChecksum, out);
      } else {
        OzecNative.checksumWindowsArray(type, array, offset, n, bytesPerChecksum, out);
      }
    }
    return out;
  }
}
